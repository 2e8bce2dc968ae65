"""What the inputs of tests/localize_cases.py reach, and the restatement tests/localize_restate.py against an independent brute
force in numpy (all candidates as one table, grouped by (frame, row), then by (frame, point)).  No GPU:
tests/test_localize_gpu.py holds the device to the restatement.  The last test needs the built library only."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as lc
import localize_restate as lr


def _all_cases():
    return lc.census() + [c for c, _ in lc.hub_cases()] + [lc.random_case()[0]]


def _brute_force(c, use_keep, use_status):
    """-> (row_point N, corr_node list) from vector operations only."""
    F, cap = c["n_frames"], c["cap"]
    N, n_points = F * cap, len(c["point_xyz"])
    cnt = np.clip(c["counts"].astype(np.int64), 0, cap)
    q, t = c["pair_q"].astype(np.int64), c["pair_t"].astype(np.int64)
    ok_pair = (q >= 0) & (q < F) & (t >= 0) & (t < F) & (q != t)
    qs, ts = np.where(ok_pair, q, 0), np.where(ok_pair, t, 0)
    i = np.arange(cap)[None, :]
    j = c["idx1"].astype(np.int64)
    ok = ok_pair[:, None] & (i < cnt[qs][:, None]) & (j >= 0) & (j < cnt[ts][:, None])
    if use_keep:
        ok &= c["keep"] != 0
    cand = c["node_point"].astype(np.int64)[np.where(ok, ts[:, None] * cap + j, 0)]
    ok &= (cand >= 0) & (cand < n_points)
    if use_status:
        ok &= c["status"][np.where(ok, cand, 0)] == 0
    node = (qs[:, None] * cap + i)[ok]
    cand = cand[ok]
    lo, hi = np.full(N, n_points, np.int64), np.full(N, -1, np.int64)
    np.minimum.at(lo, node, cand)
    np.maximum.at(hi, node, cand)
    exists = (np.arange(N) % cap) < cnt[np.arange(N) // cap]
    row_point = np.full(N, lr.NO_ROW, np.int64)
    row_point[exists] = lr.NO_POINT
    row_point[exists & (hi >= 0) & (lo != hi)] = lr.AMBIGUOUS
    claim = exists & (hi >= 0) & (lo == hi)
    frame_point = (np.arange(N) // cap) * (n_points + 1) + lo
    _, inverse, number = np.unique(frame_point[claim], return_inverse=True, return_counts=True)
    alone = number[inverse] == 1
    row_point[np.flatnonzero(claim)[alone]] = lo[claim][alone]
    row_point[np.flatnonzero(claim)[~alone]] = lr.SHARED
    return row_point, np.flatnonzero(row_point >= 0).tolist()


@pytest.mark.parametrize("use_keep,use_status", [(True, True), (False, False), (True, False)])
def test_restatement_equals_the_brute_force(use_keep, use_status):
    for c in _all_cases():
        e = lc.restate(c, use_keep, use_status)
        row_point, corr = _brute_force(c, use_keep, use_status)
        assert e["row_point"] == row_point.tolist(), c["name"]
        assert e["corr_node"][:e["totals"][0]] == corr and e["totals"][0] == len(corr), c["name"]
        assert e["totals"][1] == (row_point == lr.AMBIGUOUS).sum() and e["totals"][2] == (row_point == lr.SHARED).sum(), c["name"]
        assert e["totals"][3] == len({n // c["cap"] for n in corr}), c["name"]


def test_census_reaches_every_code_and_all_four_totals():
    codes, totals = set(), np.zeros(4, np.int64)
    for c in lc.census():
        for flags in ((True, True), (False, False)):
            e = lc.restate(c, *flags)
            codes |= {min(v, 0) for v in e["row_point"]}
            totals += e["totals"]
    assert codes == {0, lr.NO_POINT, lr.AMBIGUOUS, lr.NO_ROW, lr.SHARED}
    assert (totals > 0).all()
    by_name = {c["name"]: c for c in lc.census()}
    cap = lc.CAP
    row = lambda e, f, i: e["row_point"][f * cap + i]

    e = lc.restate(by_name["correspondence_and_no_point"])
    assert e["totals"] == [1, 0, 0, 1] and e["corr_node"][0] == 3 * cap and row(e, 3, 1) == row(e, 3, 2) == lr.NO_POINT
    assert e["offsets"] == [0, 0, 0, 0, 1, 1, 1] and e["xyz"][0] == tuple(by_name["correspondence_and_no_point"]["point_xyz"][0])
    e = lc.restate(by_name["two_pairs_disagree"])
    assert e["totals"] == [1, 2, 0, 1] and row(e, 3, 0) == row(e, 4, 1) == lr.AMBIGUOUS and row(e, 3, 4) == 4
    e = lc.restate(by_name["two_pairs_agree"])
    assert e["totals"] == [1, 0, 0, 1] and row(e, 3, 0) == 2
    e = lc.restate(by_name["same_pair_twice"])
    assert e["totals"] == [1, 0, 0, 1] and row(e, 3, 1) == 1
    e = lc.restate(by_name["many_to_one_inside_one_pair"])
    assert e["totals"] == [1, 0, 5, 1] and [row(e, 3, i) for i in range(6)] == [lr.SHARED, lr.SHARED, 2] + [lr.SHARED] * 3
    e = lc.restate(by_name["many_to_one_through_two_map_frames"])
    assert e["totals"] == [0, 0, 2, 0] and row(e, 3, 0) == row(e, 3, 1) == lr.SHARED
    e = lc.restate(by_name["same_point_from_rows_of_different_frames"])
    assert e["totals"] == [3, 0, 0, 3] and e["corr_node"][:3] == [3 * cap, 4 * cap + 5, 5 * cap + 7] and e["offsets"] == [0, 0, 0, 0, 1, 2, 3]
    e = lc.restate(by_name["ambiguous_row_claims_nothing"])
    assert e["totals"] == [1, 1, 0, 1] and row(e, 3, 0) == lr.AMBIGUOUS and row(e, 3, 1) == 0
    e = lc.restate(by_name["candidate_at_and_past_n_points"])
    assert e["totals"] == [1, 0, 0, 1] and row(e, 3, 0) == lc.N_POINTS - 1 and all(row(e, 3, i) == lr.NO_POINT for i in range(1, 8))
    c = by_name["status_other_than_ok"]
    assert lc.restate(c, True, True)["totals"] == [2, 0, 0, 1] and lc.restate(c, True, False)["totals"] == [6, 0, 0, 1]
    assert [row(lc.restate(c), 3, i) for i in range(6)] == [0, lr.NO_POINT, lr.NO_POINT, 3, lr.NO_POINT, lr.NO_POINT]
    e = lc.restate(by_name["idx1_out_of_range"])
    assert e["totals"] == [1, 0, 0, 1] and e["corr_node"][0] == 3 * cap + 4
    e = lc.restate(by_name["query_row_at_the_count"])
    assert e["totals"] == [1, 0, 0, 1] and row(e, 3, 2) == 2 and row(e, 3, 3) == lr.NO_ROW
    e = lc.restate(by_name["clamped_and_empty_counts"])
    assert e["totals"] == [2, 0, 0, 2] and e["corr_node"][:2] == [3 * cap + 7, 5 * cap + 6] and row(e, 3, 0) == lr.NO_POINT
    assert e["row_point"][:cap] == [lr.NO_ROW] * cap and e["row_point"][4 * cap:5 * cap] == [lr.NO_ROW] * cap
    e = lc.restate(by_name["pair_index_out_of_range"])
    assert e["totals"] == [1, 0, 0, 1] and row(e, 4, 1) == 1 and row(e, 3, 1) == lr.NO_POINT
    e = lc.restate(by_name["pair_of_a_frame_with_itself"])
    assert e["totals"] == [1, 0, 0, 1] and row(e, 3, 5) == 5 and row(e, 3, 0) == row(e, 0, 0) == lr.NO_POINT
    c = by_name["keep_zero"]
    assert lc.restate(c, True)["totals"] == [2, 0, 0, 1] and lc.restate(c, False)["totals"] == [1, 1, 0, 1]
    e = lc.restate(by_name["query_and_train_at_once"])
    assert e["totals"] == [3, 0, 0, 3] and row(e, 3, 0) == 0 and row(e, 4, 0) == 1 and row(e, 0, 2) == 1
    e = lc.restate(by_name["no_candidates_at_all"])
    assert e["totals"] == [0, 0, 0, 0] and set(e["row_point"]) == {lr.NO_POINT}


def test_larger_cases_reach_what_they_are_for():
    cases = lc.hub_cases()
    c, e = cases[0]
    assert e["totals"] == [1, 0, 0, 1] and e["row_point"][256 * 2] == 7 and e["offsets"][-2:] == [0, 1]
    for c, e in cases[1:]:
        assert e["totals"] == [0, 1, 0, 0] and e["row_point"][256 * 2] == lr.AMBIGUOUS, c["name"]
    c = lc.random_case()[0]
    assert c["n_frames"] * c["cap"] == 5120 and len(c["pair_q"]) == 120
    for e in lc.random_case()[1:]:  # the GPU test cannot pass vacuously
        print("random case: totals", e["totals"])
        assert e["totals"][0] >= 60 and e["totals"][1] >= 1 and e["totals"][2] >= 1


def test_properties_of_every_output():
    for c in _all_cases():
        for flags in ((True, True), (False, False)):
            e = lc.restate(c, *flags)
            F, cap = c["n_frames"], c["cap"]
            N, n_corr = F * cap, e["totals"][0]
            for k in ("row_point", "corr_node", "xyz", "xy"):
                assert len(e[k]) == N, (c["name"], k)
            assert len(e["offsets"]) == F + 1 and len(e["totals"]) == 4
            node = e["corr_node"]
            assert all(a < b for a, b in zip(node[:n_corr], node[1:n_corr])), c["name"]  # strictly ascending
            assert node[n_corr:] == [-1] * (N - n_corr) and e["xy"][n_corr:] == [(0.0, 0.0)] * (N - n_corr)
            assert e["xyz"][n_corr:] == [(0.0, 0.0, 0.0)] * (N - n_corr)
            assert e["offsets"][0] == 0 and e["offsets"][F] == n_corr and all(a <= b for a, b in zip(e["offsets"], e["offsets"][1:]))
            seen = set()
            for f in range(F):
                for k in range(e["offsets"][f], e["offsets"][f + 1]):
                    assert node[k] // cap == f and e["row_point"][node[k]] >= 0
                    assert (f, e["row_point"][node[k]]) not in seen  # a frame sees a point through one row only
                    seen.add((f, e["row_point"][node[k]]))
                    assert e["xyz"][k] == tuple(c["point_xyz"][e["row_point"][node[k]]].tolist())
            assert sum(v >= 0 for v in e["row_point"]) == n_corr
            inl = [k % 3 == 0 for k in range(N)]
            back = lr.scatter(node, n_corr, inl, N)
            assert sum(back) == sum(inl[:n_corr]) and all(back[node[k]] == inl[k] for k in range(n_corr))


def test_library_exports_both_entries_and_they_reject_a_null_context():
    """No device is touched: the context is checked before anything else."""
    from gslam_amd import hip
    assert "gh_pnp_gather_pairs_dev" not in hip.MISSING and "gh_localize_pairs_dev" not in hip.MISSING
    assert (hip.GH_LOC_NO_POINT, hip.GH_LOC_AMBIGUOUS, hip.GH_LOC_NO_ROW, hip.GH_LOC_SHARED) == (lr.NO_POINT, lr.AMBIGUOUS, lr.NO_ROW, lr.SHARED)
    one = C.c_double(1.0)
    gather = [None, None, None, 1, 1, None, None, 0, None, None, None, 0, None, None, one, one, one, one]
    assert hip.lib.gh_pnp_gather_pairs_dev(*gather, *([None] * 6)) == 1  # GH_ERR_ARG
    assert hip.lib.gh_localize_pairs_dev(*gather, one, C.c_uint64(1), 63, None, 0, one, *([None] * 12)) == 1


def test_wide_case_reaches_every_verdict_past_the_second_trip_of_the_flags_kernel():
    """tests/map_wide_cases.py: N + 1 > 1024 * 256; correspondences, AMBIGUOUS and SHARED nodes -- which loc_flags counts -- past
    node 262144."""
    import map_wide_cases as wide
    c = wide.localize_case()
    assert c["n_frames"] * c["cap"] + 1 > wide.SECOND_TRIP
    e = wide.localize_restated()
    high = e["row_point"][wide.SECOND_TRIP + 1:]
    assert high.count(lr.AMBIGUOUS) == 3 and high.count(lr.SHARED) == 6 and sum(v >= 0 for v in high) == 3 * 17 - 1  # (node 262144 itself is left out)
    assert e["totals"] == [4 * 17, 4, 8, 4]
    assert wide.localize_restated(False, False)["totals"] == [4 * 17, 8, 8, 4]
