"""Plain numpy restatement of the row-band matcher (bf_match_band_pairs_kernel, oracle_bf_match_band) and of the match
mask (match_mask_kernel, oracle_match_mask), written from their contracts and not from either implementation:

    band      = float32(size_i) * float32(band_per_size)            one float32 multiply
    dy        = abs(float32(y_i) - float32(y_j))                     one float32 subtract
    candidate = dy <= band                                           NaN on either side is never a candidate
    distance  = popcount of the XOR of the two 32-byte rows; idx1 = first minimum over the candidates, d2 = minimum over
                the candidates other than idx1; no candidate: -1 / 65535 / 65535, one candidate: d2 = 65535
    keep      = j >= 0 and d1 <= max_dist, and d1 * den < num * d2 when num > 0, and j < nt and back[j] == i when
                cross-checking (Python integers)

`rule` selects a deliberately WRONG variant; the census of tests/test_band_mask_adversarial_oracle.py uses them to show
that each class separates the contract from it: "band64" multiplies in float64 (= a fused multiply-compare), "dy64"
subtracts in float64, "lt" compares with '<', "open" ignores the band, "leak" lets an out-of-band row into d2."""
import numpy as np

NONE_IDX, NONE_D = -1, 65535
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def hamming(q, t):
    """nq x 32 and nt x 32 uint8 -> nq x nt int32 bit differences."""
    q, t = np.asarray(q, np.uint8).reshape(-1, 32), np.asarray(t, np.uint8).reshape(-1, 32)
    out = np.zeros((len(q), len(t)), np.int32)
    step = max(1, (1 << 22) // max(len(q), 1))
    for j0 in range(0, len(t), step):
        x = q[:, None, :] ^ t[None, j0:j0 + step, :]
        out[:, j0:j0 + step] = _POP[x].sum(axis=2, dtype=np.int32)
    return out


def candidates(yq, sq, yt, bps, rule="f32"):
    """nq x nt bool: train row j is a candidate of query i."""
    yq, sq, yt = (np.asarray(a, np.float32) for a in (yq, sq, yt))
    bps = np.float32(bps)
    with np.errstate(invalid="ignore", over="ignore"):
        if rule == "band64":
            band = sq.astype(np.float64) * np.float64(bps)
        else:
            band = sq * bps
            assert band.dtype == np.float32
        if rule == "dy64":
            dy = np.abs(yq.astype(np.float64)[:, None] - yt.astype(np.float64)[None, :])
        else:
            dy = np.abs(yq[:, None] - yt[None, :])
            assert dy.dtype == np.float32
        if rule == "open":
            return np.ones(dy.shape, bool)
        return dy < band[:, None] if rule == "lt" else dy <= band[:, None]


def band_match(q, kq, t, kt, bps, rule="f32"):
    """One frame pair: descriptors and KeyPoint records of the query and the train rows -> idx1, d1, d2."""
    nq, nt = len(q), len(t)
    idx1, d1, d2 = np.full(nq, NONE_IDX, np.int32), np.full(nq, NONE_D, np.uint16), np.full(nq, NONE_D, np.uint16)
    if nq == 0 or nt == 0:
        return idx1, d1, d2
    cand = candidates(kq["y"], kq["size"], kt["y"], bps, rule)
    big = 1 << 20
    dist = hamming(q, t)
    D = np.where(cand, dist, big)
    j = D.argmin(axis=1)  # first occurrence of the minimum
    rows = np.arange(nq)
    best = D[rows, j]
    has = best < big
    D2 = (dist if rule == "leak" else D).copy()
    D2[rows, j] = big
    second = D2.min(axis=1)
    idx1[has] = j[has]
    d1[has] = best[has]
    has2 = has & (second < big)
    d2[has2] = second[has2]
    return idx1, d1, d2


def band_pairs(case, rule="f32", bps=None):
    """The whole call of a case of tests/band_mask_cases.py -> (P x cap) idx1, d1, d2 with the fill of rows >= nq."""
    cap, P = case["desc"].shape[1], len(case["pair_q"])
    idx1 = np.full((P, cap), NONE_IDX, np.int32)
    d1, d2 = np.full((P, cap), NONE_D, np.uint16), np.full((P, cap), NONE_D, np.uint16)
    n = np.clip(case["counts"], None, cap)
    for p, (a, b) in enumerate(zip(case["pair_q"], case["pair_t"])):
        na, nb = max(int(n[a]), 0), max(int(n[b]), 0)
        r = band_match(case["desc"][a, :na], case["kps"][a, :na], case["desc"][b, :nb], case["kps"][b, :nb],
                       case["bps"] if bps is None else bps, rule)
        idx1[p, :na], d1[p, :na], d2[p, :na] = r
    return idx1, d1, d2


def match_mask(idx1, d1, d2, back, nt, max_dist, ratio_num, ratio_den, cross_check, strict=True):
    """strict=False is the wrong '<=' ratio rule (census only)."""
    keep = np.zeros(len(idx1), np.uint8)
    for i in range(len(idx1)):
        j, a, b = int(idx1[i]), int(d1[i]), int(d2[i])
        ok = j >= 0 and a <= max_dist
        if ok and ratio_num > 0:
            ok = a * ratio_den < ratio_num * b if strict else a * ratio_den <= ratio_num * b
        if ok and cross_check:
            ok = j < nt and int(back[j]) == i
        keep[i] = 1 if ok else 0
    return keep
