"""The band matcher and match mask oracles (oracle/bf_oracle.c) on the adversarial classes of tests/band_mask_cases.py.

Census first: each class is held, with the plain numpy restatement of tests/band_mask_restate.py and not with the code
under test, to what it was built to reach: the hand-derived (idx1, d1, d2) of every planted query, rows exactly on the band
and one ulp either side of it, queries that a float64 product / a float64 difference / a '<' / a leaking second minimum
would answer differently, the ragged counts, the 16-bit index top.  Then parity: oracle_bf_match_band equals the
restatement on every row of every class, and oracle_match_mask equals the restated integer rule on every mask class at
1, 255, 256, 257 and 600 rows."""
import numpy as np
import pytest

import band_mask_cases as bc
import band_mask_restate as br

F32 = np.float32

_restated = {}


def restated(name, rule="f32"):
    if (name, rule) not in _restated:
        _restated[name, rule] = br.band_pairs(bc.band_case(name), rule)
    return _restated[name, rule]


def _differs(name, rule, rows):
    """the query rows of pair 0 among `rows` whose idx1 changes under the wrong rule"""
    a, b = restated(name)[0][0], restated(name, rule)[0][0]
    return [i for i in rows if a[i] != b[i]]


# ------------------------------------------------------------------------------------------------------------- census
@pytest.mark.parametrize("name", bc.BAND_NAMES)
def test_band_census(name):
    c = bc.band_case(name)
    cap = c["desc"].shape[1]
    idx1, d1, d2 = restated(name)
    assert c["desc"].dtype == np.uint8 and c["kps"].dtype == bc.KP_DTYPE and c["bps"].dtype == np.float32
    assert np.isnan(c["kps"]["x"]).all() and np.isnan(c["kps"]["angle"]).all()  # only y and size carry values
    for i, (j, a, b) in c["want"].items():
        assert idx1[0, i] == j and d1[0, i] == a and (b is None or d2[0, i] == b), (name, i, idx1[0, i], d1[0, i], d2[0, i])
    if name not in ("ragged", "wide_open", "index_top"):
        nq, nt = c["counts"]
        assert len(c["want"]) == nq and nq < cap and nt < cap and cap % 64 != 0
        # other queries' rows never come close: the planted group decides alone
        d = br.hamming(c["desc"][0, :nq], c["desc"][1, :nt])
        assert np.sort(d, axis=1)[:, :6].max() > 64 or nt < 6
        # the rows past the train count are exact copies of the queries (they would win if read)
        assert (br.hamming(c["desc"][0, :1], c["desc"][1, nt:nt + 1]) == 0).all()
    q = c["kps"][0]
    if name == "boundary":
        assert len(c["want"]) == 2 * len(bc.SIZES)
        for i, (j, _, _) in c["want"].items():
            band = F32(q["size"][i] * c["bps"])
            dy = np.abs(q["y"][i] - c["kps"]["y"][1, j - 1:j + 2])
            assert dy.dtype == np.float32 and dy[1] == band
            assert dy[0] == np.nextafter(band, F32(np.inf)) and dy[2] == np.nextafter(band, F32(0))
        sides = np.sign(c["kps"]["y"][1, [w[0] for w in c["want"].values()]] - q["y"][:len(c["want"])])
        assert (sides > 0).sum() == (sides < 0).sum() == len(bc.SIZES)
        everyone = list(c["want"])
        assert _differs(name, "lt", everyone) == everyone      # '<' drops the row on the band
        assert _differs(name, "open", everyone) == everyone    # any wider band takes the closest row, an ulp outside
    if name == "fp32_product":
        rows = c["kinds"]["product"]
        assert len(rows) >= 4 and _differs(name, "band64", rows) == rows and not _differs(name, "dy64", rows)
    if name == "fp32_difference":
        rows = c["kinds"]["difference"]
        assert len(rows) == 3 and _differs(name, "dy64", rows) == rows and not _differs(name, "band64", rows)
    if name == "zero_band":
        assert c["bps"] == 0 and (q["size"][c["kinds"]["zero"]] == 0).sum() >= 2
        y = c["kps"]["y"][:, :max(c["counts"])]
        assert np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()
        assert (np.abs(y[(y != 0) & np.isfinite(y)]).min() < 1.2e-38)           # a denormal y
        assert _differs(name, "open", c["kinds"]["zero"][:3]) == c["kinds"]["zero"][:3]
        with np.errstate(invalid="ignore"):
            assert np.isnan(F32(np.inf) * c["bps"]) and idx1[0, c["kinds"]["nan_band"][0]] == -1
    if name == "none_one_two":
        k = c["kinds"]
        assert (idx1[0, k["none"]] == -1).all() and (d2[0, k["one"]] == 65535).all() and (idx1[0, k["one"]] >= 0).all()
        two = k["two"][0]
        assert d1[0, two] == d2[0, two] and idx1[0, two] == c["want"][two][0]
        leak = br.band_pairs(c, "leak")
        for kind in ("dup_before", "dup_after", "dup_only"):  # the masked duplicate would become d2 / idx1
            i = k[kind][0]
            assert leak[2][0, i] == d1[0, i] != d2[0, i]
        assert _differs(name, "open", k["dup_before"] + k["dup_only"] + k["none"]) == k["dup_before"] + k["dup_only"] + k["none"]
    if name == "nonfinite":
        y, s = c["kps"]["y"], c["kps"]["size"]
        assert np.isnan(y[0, :c["counts"][0]]).any() and np.isnan(y[1, :c["counts"][1]]).any()
        assert np.isposinf(s[0]).any() and (s[0] < 0).any() and np.isnan(s[0]).any()
        assert np.isinf(y[0, :c["counts"][0]]).any() and np.isinf(y[1, :c["counts"][1]]).any()
        for kind in ("nan_query", "neg_size", "nan_size"):
            assert (idx1[0, c["kinds"][kind]] == -1).all()
        i = c["kinds"]["inf_size"][0]
        cand = br.candidates(q["y"][i:i + 1], q["size"][i:i + 1], c["kps"]["y"][1, :c["counts"][1]], c["bps"])[0]
        yt = c["kps"]["y"][1, :c["counts"][1]]
        assert np.array_equal(cand, ~np.isnan(yt)) and np.isfinite(yt).sum() >= 8  # every finite-y row (|dy| = inf passes too)
    if name in ("ragged", "wide_open"):
        assert sorted(c["counts"].tolist()) == [0, 1, 63, 64, 65, cap, cap + 7]
        pairs = list(zip(c["pair_q"].tolist(), c["pair_t"].tolist()))
        assert any(a == b for a, b in pairs) and len(set(pairs)) < len(pairs)
        assert any(c["counts"][a] == 0 for a, _ in pairs) and any(c["counts"][b] == 0 for _, b in pairs)
    if name == "ragged":
        wide = restated("wide_open")
        valid = wide[0] >= 0
        assert valid.sum() > 3000
        changed = (idx1 != wide[0]) & valid
        assert 0.1 < changed.sum() / valid.sum() < 0.9          # the band decides a good part of the rows, not all
        assert ((idx1 == -1) & valid).sum() > 20 and ((d2 == 65535) & (idx1 >= 0)).sum() > 20
        assert (restated(name, "lt")[0] != idx1).any()
    if name == "wide_open":
        assert c["bps"] == F32(1e30) and (c["kps"]["size"] > 0).all() and np.isfinite(c["kps"]["y"]).all()
        assert all(np.array_equal(a, b) for a, b in zip(restated(name), br.band_pairs(c, "open")))
    if name == "index_top":
        assert cap == 65535 and c["counts"].tolist() == [64, 65535]
        assert (idx1[0, :63] == 65534).all() and idx1[0, 63] == 3
        assert np.array_equal(c["desc"][1, 3], c["desc"][1, 65534])
        assert (idx1[1] >= 0).sum() > 60000 and idx1[1].max() == 63


@pytest.mark.parametrize("name", list(bc.MASK_CLASSES))
def test_mask_census(name):
    kept = 0
    for nq in bc.MASK_NQ:
        for c in bc.mask_cases(name, nq):
            assert len(c["idx1"]) == nq and c["idx1"].dtype == np.int32 and c["d1"].dtype == c["d2"].dtype == np.uint16
            assert abs(c["ratio_num"]) <= 32767 and abs(c["ratio_den"]) <= 32767
            keep = br.match_mask(c["idx1"], c["d1"], c["d2"], c["back"], c["nt"], c["max_dist"], c["ratio_num"], c["ratio_den"],
                                 c["cross_check"])
            kept += int(keep.sum())
            if nq < 255:
                continue
            i1, a, b = c["idx1"].astype(np.int64), c["d1"].astype(np.int64), c["d2"].astype(np.int64)
            if name == "no_match":
                assert not keep[i1 < 0].any() and ((i1 < 0) & (a == 0)).any() and ((i1 < 0) & (a == 65535) & (b == 65535)).any()
            if name == "d2_none":
                assert (b == 65535).all() and keep.any() and (keep.all() == (c["ratio_num"] == 32767 and c["ratio_den"] == 1))
            if name == "ratio_off":
                assert c["ratio_num"] <= 0 and np.array_equal(keep, ((i1 >= 0) & (a <= c["max_dist"])).astype(np.uint8))
                assert keep[a >= b].any()  # rows the ratio test would reject
            if name == "ratio_big":
                assert max(c["ratio_num"], c["ratio_den"]) == 32767 and (a * c["ratio_den"]).max() < 2 ** 31
                assert (c["ratio_num"] * b).max() < 2 ** 31 and keep.any() and not keep.all()
            if name == "max_dist":
                assert c["max_dist"] in (0, -1, 256) and np.array_equal(keep, ((i1 >= 0) & (a <= c["max_dist"])).astype(np.uint8))
            if name == "ratio_equal":
                eq = a * c["ratio_den"] == c["ratio_num"] * b
                assert eq.any() and not keep[eq].any() and keep.any()
                loose = br.match_mask(c["idx1"], c["d1"], c["d2"], c["back"], c["nt"], c["max_dist"], c["ratio_num"],
                                      c["ratio_den"], c["cross_check"], strict=False)
                assert loose[eq].all()  # '<=' would keep them
            if name == "cross":
                past = i1 >= c["nt"]
                assert past.any() and not keep[past].any() and keep.any() and len(c["back"]) > i1.max()
                mutual = (i1 >= 0) & (c["back"][np.clip(i1, 0, None)] == np.arange(nq))
                assert mutual[past].any()                       # the back list alone would keep rows past nt
                assert (~mutual & ~past & (i1 >= 0) & (a <= c["max_dist"])).any()
            if name == "cross_off":
                assert c["back"] is None and c["cross_check"] == 0 and (i1 >= nq).any() and keep[i1 >= nq].all()
    assert kept > 0


# ------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", bc.BAND_NAMES)
def test_band_oracle_equals_restatement(oracle, name):
    c = bc.band_case(name)
    got, want = bc.oracle_pairs(oracle, c), restated(name)
    for g, w, what in zip(got, want, ("idx1", "d1", "d2")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, what, int((g != w).sum()))


def test_wide_open_is_the_plain_matcher(oracle):
    c = bc.band_case("wide_open")
    want = restated("wide_open")
    n = np.clip(c["counts"], 0, c["desc"].shape[1])
    for p, (a, b) in enumerate(zip(c["pair_q"], c["pair_t"])):
        e = oracle.bf_match(c["desc"][a, :n[a]], c["desc"][b, :n[b]])
        for g, w in zip(e, want):
            assert np.array_equal(g, w[p, :n[a]]), (p, a, b)


@pytest.mark.parametrize("name", list(bc.MASK_CLASSES))
def test_mask_oracle_equals_restatement(oracle, name):
    rows = 0
    for nq in bc.MASK_NQ:
        for c in bc.mask_cases(name, nq):
            want = br.match_mask(c["idx1"], c["d1"], c["d2"], c["back"], c["nt"], c["max_dist"], c["ratio_num"], c["ratio_den"],
                                 c["cross_check"])
            got = oracle.match_mask(c["idx1"], c["d1"], c["d2"], c["back"], c["nt"], c["max_dist"], c["ratio_num"], c["ratio_den"],
                                    c["cross_check"])
            assert np.array_equal(got, want), (name, nq, c["max_dist"], c["ratio_num"], c["ratio_den"], np.nonzero(got != want)[0][:5])
            rows += nq
    assert rows >= 2 * sum(bc.MASK_NQ)
