"""Adversarial inputs for the row-band matcher (gh_bf_match_band_pairs_dev) and the match mask (gh_match_mask_dev): the
inputs an ORB extraction never produces (tests/test_band_mask_adversarial_oracle.py takes the census of what each class
reaches and pins the oracle on it, tests/test_band_mask_adversarial_gpu.py holds the kernels to the oracle).  numpy only,
seeded.

BAND_CLASSES[name]() -> dict
    desc F x cap x 32 uint8, kps F x cap KP_DTYPE, counts F int32, pair_q / pair_t P int32, bps float32, and
    "want": {query row of pair 0: (train row or -1, d1, d2)} for the hand-built queries, "kinds": {kind: [query rows]}
Planted classes hold one query frame (0) and one train frame (1).  Every query owns a group of train rows that are its
own descriptor with a few bits flipped (rows of other groups are random, > 64 bits away), and the row the band rule has to
exclude is always the Hamming-closest of the group: a wrong inclusion changes idx1, and so does a wrong exclusion.
Only `y` and `size` of a KeyPoint take part; the other fields hold NaN / -inf / INT_MIN, which would poison a result
that read them.

MASK_CLASSES[name](nq) -> [dict(idx1, d1, d2, back (None: no back list), nt, max_dist, ratio_num, ratio_den, cross_check)]
Builders are cached: the arrays are shared and must not be written to."""
import functools

import numpy as np

from gslam_amd.orb import KP_DTYPE

CAP = 150                       # not a multiple of the 64-query wave
BPS = np.float32(2.0 / 31.0)    # the benchmark's band: +-2 px at level 0
SIZES = [np.float32(31.0 * 1.2 ** k) for k in range(8)]
F32 = np.float32

BAND_CLASSES = {}
MASK_CLASSES = {}
MASK_NQ = (1, 255, 256, 257, 600)


def _register(table, name):
    def deco(fn):
        table[name] = functools.lru_cache(maxsize=None)(fn)
        return fn
    return deco


def blank_kps(shape):
    k = np.zeros(shape, KP_DTYPE)
    k["x"], k["angle"], k["response"] = np.nan, np.nan, -np.inf
    k["octave"], k["class_id"] = np.iinfo(np.int32).min, 0x55555555
    k["y"], k["size"] = 1.0e6, 31.0
    return k


def _flip(row, bits):
    out = row.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def _bits(n, first=0):
    return tuple(range(first, first + n))


def _planted(specs, bps, seed, cap=CAP):
    """specs: [(kind, y_q, size_q, [(y_t, flipped bits), ...], want)] with want = (row within the group or -1, d1, d2; None: not hand-derived)."""
    rng = np.random.default_rng(seed)
    nq, nt = len(specs), sum(len(s[3]) for s in specs)
    assert nq <= cap and nt <= cap
    desc = rng.integers(0, 256, (2, cap, 32), dtype=np.uint8)
    kps = blank_kps((2, cap))
    want, kinds, j = {}, {}, 0
    for i, (kind, yq, sq, rows, w) in enumerate(specs):
        kps["y"][0, i], kps["size"][0, i] = yq, sq
        for yt, bits in rows:
            desc[1, j] = _flip(desc[0, i], bits)
            kps["y"][1, j] = yt
            j += 1
        first = j - len(rows)
        want[i] = (first + w[0] if w[0] >= 0 else -1, w[1], w[2])
        kinds.setdefault(kind, []).append(i)
    # rows past the counts: exact copies of the queries on the queries' rows, which would win if they were read
    desc[1, nt:nt + min(nq, cap - nt)] = desc[0, :min(nq, cap - nt)]
    kps["y"][1, nt:nt + min(nq, cap - nt)] = kps["y"][0, :min(nq, cap - nt)]
    kps["size"][1, nt:] = np.inf
    return dict(desc=desc, kps=kps, counts=np.array([nq, nt], np.int32), pair_q=np.array([0], np.int32),
                pair_t=np.array([1], np.int32), bps=F32(bps), want=want, kinds=kinds)


def exact_rows(band, side):
    """(y_q, [y_t at dy just above the band, at dy == band, at dy just below]) in float32 with every difference exact;
    side +1: the train rows lie above the query, -1: below.  All values share the grid of the band's ulp; where a band at
    the bottom of its binade leaves no positive y_q for side +1 the query lies below zero."""
    band = F32(band)
    targets = [np.nextafter(band, F32(np.inf)), band, np.nextafter(band, F32(0))]
    g = float(np.spacing(targets[2]))
    top = 2.0 ** np.ceil(np.log2(float(targets[0])) + 1e-9)
    tries = [(4000 + j) * g for j in range(3, 2048)] + [-j * g for j in range(3, 2048)] if side > 0 else \
        [top - j * g for j in range(3, 4096)]
    for yq in tries:
        yts = [yq + side * float(t) for t in targets]
        f = [F32(v) for v in [yq] + yts]
        if all(float(a) == b for a, b in zip(f, [yq] + yts)) and \
                all(np.abs(F32(f[0] - y)) == t for y, t in zip(f[1:], targets)):
            return f[0], f[1:]
    raise AssertionError(("no exact rows", band, side))


@_register(BAND_CLASSES, "boundary")
def boundary():
    """Per level size 31 * 1.2^k and side: the closest row one ulp outside the band, then a row exactly on it (wins),
    then one an ulp inside (second)."""
    specs = []
    for s in SIZES:
        for side in (+1, -1):
            yq, (above, on, below) = exact_rows(F32(s * BPS), side)
            specs.append(("boundary", yq, s, [(above, ()), (on, _bits(1)), (below, _bits(2))], (1, 1, 2)))
    return _planted(specs, BPS, 201)


def _rounded_up_sizes():
    return [s for s in SIZES if float(F32(s * BPS)) > float(s) * float(BPS)]


@_register(BAND_CLASSES, "fp32_product")
def fp32_product():
    """The fp32 rule, the multiply: for the level sizes where float32(size * bps) lies above the exact product the closest
    row sits exactly on the float32 band, on either side of the query; a float64 or fused product leaves it out."""
    specs = []
    ups = _rounded_up_sizes()
    assert len(ups) >= 2
    for s in ups:
        for side in (+1, -1):
            yq, (_, on, _) = exact_rows(F32(s * BPS), side)
            inside = F32(yq + F32(side) * F32(0.5))
            specs.append(("product", yq, s, [(on, ()), (inside, _bits(3))], (0, 0, 3)))
    return _planted(specs, BPS, 202)


@_register(BAND_CLASSES, "fp32_difference")
def fp32_difference():
    """The fp32 rule, the subtraction: the product is exact (bps = 1/16) and y_t = -/+ 2^-40 lifts the exact difference
    above the band while float32(y_q - y_t) is the band itself; a float64 difference leaves the closest row out."""
    specs = []
    for s, sign in ((F32(37.0), 1), (F32(49.5), -1), (F32(127.0), 1)):
        band = F32(s * F32(0.0625))
        specs.append(("difference", F32(sign * band), s, [(F32(-sign * 2.0 ** -40), ()), (F32(sign * band * F32(0.5)), _bits(3))],
                      (0, 0, 3)))
    return _planted(specs, F32(0.0625), 203)


@_register(BAND_CLASSES, "zero_band")
def zero_band():
    """band_per_size = 0: only rows on the query's own y remain (-0.0 equals 0.0; a denormal step away does not), with
    size 0 and size 31; size = inf gives 0 * inf = NaN, no candidate at all."""
    tiny = np.nextafter(F32(0), F32(1))
    up, dn = np.nextafter(F32(57.25), F32(np.inf)), np.nextafter(F32(57.25), F32(0))
    specs = [
        ("zero", F32(0.0), F32(0), [(tiny, ()), (F32(-0.0), _bits(1)), (F32(0.0), _bits(2)), (-tiny, ())], (1, 1, 2)),
        ("zero", F32(-0.0), F32(31), [(tiny, ()), (F32(0.0), _bits(2)), (F32(-0.0), _bits(1))], (2, 1, 2)),
        ("zero", F32(57.25), F32(0), [(up, ()), (F32(57.25), _bits(1)), (dn, ()), (F32(57.25), _bits(2))], (1, 1, 2)),
        ("zero", F32(300.5), F32(-0.0), [(F32(300.5), _bits(4))], (0, 4, 65535)),
        ("nan_band", F32(811.0), F32(np.inf), [(F32(811.0), ())], (-1, 65535, 65535)),
    ]
    return _planted(specs, F32(0), 204)


@_register(BAND_CLASSES, "none_one_two")
def none_one_two():
    """size 31 (band 2) at y = 100 * group: no candidate, exactly one, two at equal distance, an exact duplicate of the
    best row out of band in front of it / behind it, and an out-of-band duplicate in front of the only candidate."""
    s = F32(31)
    specs = [
        ("none", F32(100), s, [(F32(105), ()), (F32(93), _bits(1))], (-1, 65535, 65535)),
        ("one", F32(200), s, [(F32(205), ()), (F32(201), _bits(4))], (1, 4, 65535)),
        ("two", F32(300), s, [(F32(300.5), _bits(3)), (F32(299), _bits(3, 5))], (0, 3, 3)),
        ("dup_before", F32(400), s, [(F32(409), _bits(2)), (F32(401), _bits(2)), (F32(398.5), _bits(6))], (1, 2, 6)),
        ("dup_after", F32(500), s, [(F32(501), _bits(2)), (F32(491), _bits(2)), (F32(498.5), _bits(6))], (0, 2, 6)),
        ("dup_only", F32(600), s, [(F32(610), _bits(1)), (F32(600), _bits(1))], (1, 1, 65535)),
        ("one", F32(700), s, [(F32(700), ()), (F32(702.5), ())], (0, 0, 65535)),
    ]
    return _planted(specs, BPS, 205)


@_register(BAND_CLASSES, "nonfinite")
def nonfinite():
    """NaN y on either side, +inf size (every finite-y row is a candidate, an infinite one too unless inf - inf), negative
    and NaN size (nothing is), infinite y against infinite y."""
    s, inf, nan = F32(31), F32(np.inf), F32(np.nan)
    specs = [
        ("inf_size", F32(100), inf, [(nan, ()), (F32(3e38), _bits(1)), (F32(-1e30), _bits(2))], (1, 1, 2)),
        ("inf_size", F32(150), inf, [(inf, _bits(1)), (F32(-2e38), _bits(2))], (0, 1, 2)),
        ("nan_query", nan, s, [(F32(200), ()), (nan, ())], (-1, 65535, 65535)),
        ("nan_query", nan, inf, [(F32(250), ())], (-1, 65535, 65535)),
        ("neg_size", F32(300), F32(-31), [(F32(300), ())], (-1, 65535, 65535)),
        ("nan_size", F32(400), nan, [(F32(400), ())], (-1, 65535, 65535)),
        ("inf_y", inf, s, [(inf, ()), (F32(500), _bits(1))], (-1, 65535, 65535)),
        ("inf_y", inf, inf, [(inf, ()), (-inf, _bits(2)), (F32(5), _bits(1))], (2, 1, 2)),
        ("inf_y", -inf, inf, [(-inf, ()), (inf, _bits(3))], (1, 3, None)),
        ("nan_train", F32(600), s, [(nan, ()), (F32(601), _bits(3))], (1, 3, 65535)),
    ]
    return _planted(specs, BPS, 206)


def _ragged_frames(seed, bps):
    """Seven frames of one scene (shared base descriptors, shuffled, a few bits flipped) with counts 0, 1, 63, 64, 65, cap
    and cap + 7; y on a coarse lattice plus offsets around the band; every frame pair, self pairs included, one repeated."""
    rng = np.random.default_rng(seed)
    counts = np.array([0, 1, 63, 64, 65, CAP, CAP + 7], np.int32)
    F = len(counts)
    base = rng.integers(0, 256, (CAP, 32), dtype=np.uint8)
    base_y = (10.0 * rng.integers(0, 12, CAP)).astype(np.float32)
    desc = np.zeros((F, CAP, 32), np.uint8)
    kps = blank_kps((F, CAP))
    offs = np.array([0, 0, 1, -1, 2, -2.5, 3, -6, 2.0625, -2.0625], np.float32)
    for f in range(F):
        perm = rng.permutation(CAP)
        flips = (rng.random((CAP, 256)) < 0.02).astype(np.uint8)
        desc[f] = base[perm] ^ np.packbits(flips, axis=1, bitorder="little")
        kps["y"][f] = base_y[perm] + offs[rng.integers(0, len(offs), CAP)]
        kps["size"][f] = np.array(SIZES, np.float32)[rng.integers(0, 8, CAP)]
    pq, pt = np.meshgrid(np.arange(F), np.arange(F), indexing="ij")
    pair_q = np.append(pq.reshape(-1), 5).astype(np.int32)
    pair_t = np.append(pt.reshape(-1), 6).astype(np.int32)
    return dict(desc=desc, kps=kps, counts=counts, pair_q=pair_q, pair_t=pair_t, bps=F32(bps), want={}, kinds={})


@_register(BAND_CLASSES, "ragged")
def ragged():
    return _ragged_frames(207, BPS)


@_register(BAND_CLASSES, "wide_open")
def wide_open():
    """The ragged frames under band_per_size = 1e30: every row is a candidate, the plain pair matcher's result."""
    return _ragged_frames(207, 1e30)


@_register(BAND_CLASSES, "index_top")
def index_top():
    """cap = 65535, counts 64 and 65535: the best row of every query is the last one the 16-bit index field can name
    (65534), its exact duplicate at row 3 is out of band; query 63 sits on row 3's y instead.  Both directions."""
    cap = 65535
    rng = np.random.default_rng(208)
    desc = rng.integers(0, 256, (2, cap, 32), dtype=np.uint8)
    kps = blank_kps((2, cap))
    root = desc[1, cap - 1].copy()
    desc[1, 3] = root
    for i in range(64):
        desc[0, i] = _flip(root, _bits(i % 7, 8 * (i % 5)))
    kps["y"][0, :64], kps["size"][0, :64] = 50.0, 31.0
    kps["y"][1], kps["size"][1] = (50.0 + (np.arange(cap) % 5) * 0.5 - 1.0).astype(np.float32), SIZES[1]
    kps["y"][1, 3] = 40.0
    kps["y"][1, cap - 1] = 51.5
    kps["y"][0, 63] = 41.5
    want = {i: (cap - 1, i % 7, None) for i in range(63)}
    want[63] = (3, 63 % 7, 65535)
    return dict(desc=desc, kps=kps, counts=np.array([64, cap], np.int32), pair_q=np.array([0, 1], np.int32),
                pair_t=np.array([1, 0], np.int32), bps=BPS, want=want, kinds={})


def band_case(name):
    return BAND_CLASSES[name]()


def oracle_pairs(oracle, case):
    """oracle_bf_match_band per pair of the call, in the (P x cap) layout with the fill of rows >= nq."""
    cap, P = case["desc"].shape[1], len(case["pair_q"])
    idx1 = np.full((P, cap), -1, np.int32)
    d1, d2 = np.full((P, cap), 65535, np.uint16), np.full((P, cap), 65535, np.uint16)
    n = np.clip(case["counts"], 0, cap)
    for p, (a, b) in enumerate(zip(case["pair_q"], case["pair_t"])):
        na, nb = int(n[a]), int(n[b])
        r = oracle.bf_match_band(case["desc"][a, :na], case["kps"][a, :na], case["desc"][b, :nb], case["kps"][b, :nb], case["bps"])
        idx1[p, :na], d1[p, :na], d2[p, :na] = r
    return idx1, d1, d2


BAND_NAMES = list(BAND_CLASSES)
SMALL_BAND_NAMES = [n for n in BAND_NAMES if n != "index_top"]


# ------------------------------------------------------------------------------------------------------- match mask
def _mask_case(rows, nq, shift, nt=0, back=None, max_dist=256, num=0, den=1, cross=0):
    """rows: [(idx1, d1, d2)] repeated to nq rows starting at `shift`; back: callable(i, j, nt) -> back entry of row j for
    the rows whose match is j, or None for a call without a back list."""
    pick = [rows[(i + shift) % len(rows)] for i in range(nq)]
    idx1 = np.array([r[0] for r in pick], np.int32)
    d1 = np.array([r[1] for r in pick], np.uint16)
    d2 = np.array([r[2] for r in pick], np.uint16)
    return dict(idx1=idx1, d1=d1, d2=d2, back=back, nt=nt, max_dist=max_dist, ratio_num=num, ratio_den=den, cross_check=cross)


@_register(MASK_CLASSES, "no_match")
def mask_no_match(nq):
    """idx1 = -1 with the matcher's 65535 / 65535 and with distances that would pass every test."""
    rows = [(-1, 65535, 65535), (-1, 0, 100), (4, 10, 100), (-1, 30, 65535), (-7, 0, 200)]
    return [_mask_case(rows, nq, s, max_dist=m, num=7, den=10) for s, m in ((0, 256), (1, 65535), (2, 50))]


@_register(MASK_CLASSES, "d2_none")
def mask_d2_none(nq):
    """One candidate only (d2 = 65535) under the ratio test, up to the largest factor whose product stays inside int."""
    rows = [(5, 30, 65535), (0, 256, 65535), (9, 0, 65535), (3, 65535, 65535)]
    return [_mask_case(rows, nq, s, max_dist=65535, num=n, den=d) for s, (n, d) in enumerate(((7, 10), (32767, 32767), (1, 32767), (32767, 1)))]


@_register(MASK_CLASSES, "ratio_off")
def mask_ratio_off(nq):
    """ratio_num = 0 and negative: the ratio test is off; rows it would reject stay."""
    rows = [(2, 50, 50), (2, 50, 0), (1, 60, 10), (0, 40, 65535), (6, 257, 300)]
    return [_mask_case(rows, nq, s, num=n, den=d) for s, (n, d) in enumerate(((0, 1), (0, 0), (-3, 10), (-32767, -5)))]


@_register(MASK_CLASSES, "ratio_big")
def mask_ratio_big(nq):
    """ratio_num and ratio_den up to 32767 against distances up to 65535."""
    rows = [(1, 100, 100), (1, 99, 100), (1, 65535, 65535), (1, 65534, 65535), (1, 1, 65535), (1, 2, 1), (1, 0, 0), (1, 0, 1)]
    return [_mask_case(rows, nq, s, max_dist=65535, num=n, den=d)
            for s, (n, d) in enumerate(((32767, 32767), (32767, 1), (1, 32767), (32766, 32767), (32767, 32766)))]


@_register(MASK_CLASSES, "max_dist")
def mask_max_dist(nq):
    rows = [(3, 0, 9), (3, 1, 9), (3, 256, 300), (3, 257, 300), (3, 255, 300), (-1, 0, 9)]
    return [_mask_case(rows, nq, s, max_dist=m) for s, m in enumerate((0, -1, 256))]


@_register(MASK_CLASSES, "ratio_equal")
def mask_ratio_equal(nq):
    """d1 * den == num * d2 exactly: the rule is the strict '<'."""
    rows = [(8, 35, 50), (8, 34, 50), (8, 36, 50), (8, 70, 100), (8, 7, 10), (8, 0, 0), (8, 69, 100)]
    return [_mask_case(rows, nq, s, num=7, den=10) for s in (0, 1, 3)]


@_register(MASK_CLASSES, "cross")
def mask_cross(nq):
    """Cross-check with nt below some of the matches: rows whose match is >= nt fall without back[j] deciding (the back
    list given to the call still covers every j and says "mutual" there, so a kernel that ignored nt would keep them)."""
    out = []
    for s, nt in ((0, 4), (1, max(nq // 2, 1)), (2, nq + 3)):
        rows = [(0, 10, 90), (1, 10, 90), (nt - 1, 10, 90), (nt, 10, 90), (nt + 2, 10, 90), (2, 300, 400), (-1, 65535, 65535)]
        c = _mask_case(rows, nq, s, nt=nt, num=7, den=10, cross=1)
        n_back = max(int(c["idx1"].max()) + 1, nt, 1)
        back = np.full(n_back, -1, np.int32)
        for i in range(nq):  # the last writer of an entry is mutual, earlier rows with the same match are not
            if c["idx1"][i] >= 0 and i % 3 != 1:
                back[c["idx1"][i]] = i
        c["back"] = back
        out.append(c)
    return out


@_register(MASK_CLASSES, "cross_off")
def mask_cross_off(nq):
    """cross_check = 0: no back list is read (the call passes a null pointer), nt = 0 does not matter."""
    rows = [(0, 10, 90), (5, 10, 12), (nq + 9, 10, 90), (-1, 65535, 65535)]
    return [_mask_case(rows, nq, s, nt=0, num=n, den=10) for s, n in ((0, 7), (1, 0))]


def mask_cases(name, nq):
    return MASK_CLASSES[name](nq)
