"""What the inputs of tests/track_link_cases.py reach, and the restatement tests/track_link_restate.py against
scipy.sparse.csgraph.connected_components.  No GPU: tests/test_track_link_gpu.py holds the device to the restatement."""
import numpy as np
import pytest

import track_link_cases as lc
import track_link_restate as lr


def _all_cases():
    return lc.census() + [lc.chain(), lc.hub(), lc.hub(True), lc.random_case()[0]]


def _scipy_partition(c, use_inlier):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    N = c["n_frames"] * c["cap"]
    e = lr.edges(c["counts"].tolist(), c["n_frames"], c["cap"], c["pair_q"].tolist(), c["pair_t"].tolist(),
                 c["idx1"].reshape(-1).tolist(), c["inlier"].reshape(-1).tolist() if use_inlier else None)
    a = np.array(e, np.int64).reshape(-1, 2)
    g = coo_matrix((np.ones(len(a), np.int8), (a[:, 0], a[:, 1])), shape=(N, N))
    _, lab = connected_components(g, directed=False)
    exists = (np.arange(N) % c["cap"]) < np.clip(c["counts"], 0, c["cap"])[np.arange(N) // c["cap"]]
    groups = {}
    for n in np.flatnonzero(exists).tolist():
        groups.setdefault(int(lab[n]), []).append(n)
    return sorted(groups.values())


@pytest.mark.parametrize("use_inlier", [True, False])
def test_components_equal_scipy_as_partitions_and_labels_are_the_smallest_id(use_inlier):
    for c in _all_cases():
        comps = lc.restate(c, use_inlier)["components"]
        assert sorted(comps.values()) == _scipy_partition(c, use_inlier), c["name"]
        assert all(label == min(nodes) for label, nodes in comps.items()), c["name"]


def test_census_reaches_every_code_and_both_counters():
    codes, conflicts, shorts, lengths = set(), 0, 0, set()
    for c in lc.census():
        for mv in (2, 3):
            e = lc.restate(c, True, mv)
            codes |= {min(v, 0) for v in e["node_point"]}
            conflicts += e["totals"][2]
            shorts += e["totals"][3]
            lengths |= set(e["point_len"][:e["totals"][1]])
    assert codes == {0, lr.SHORT, lr.CONFLICT, lr.NO_ROW}
    assert conflicts > 0 and shorts > 0 and {2, 3, 6} <= lengths
    by_name = {c["name"]: c for c in lc.census()}
    e = lc.restate(by_name["many_to_one_drops_the_chain"])
    assert e["totals"] == [2, 1, 1, 0] and sum(v == lr.CONFLICT for v in e["node_point"]) == 7  # frames 0 (twice), 1 .. 5
    e = lc.restate(by_name["conflict_through_a_third_frame"])
    assert e["totals"][:3] == [0, 0, 1]
    e = lc.restate(by_name["min_views_3"])
    assert e["totals"] == [3, 1, 0, 2]
    e = lc.restate(by_name["idx1_out_of_range"])
    assert e["totals"][:2] == [2, 1] and e["obs_node"][:2] == [4, 8 + 4]
    e = lc.restate(by_name["query_row_at_the_count"])
    assert e["totals"][:2] == [2, 1] and e["obs_node"][:2] == [2, 8 + 2] and e["node_point"][3] == lr.NO_ROW
    e = lc.restate(by_name["clamped_and_empty_counts"])
    assert e["totals"][:2] == [4, 2] and e["obs_node"][:4] == [15, 23, 38, 46] and e["node_point"][:8] == [lr.NO_ROW] * 8
    e = lc.restate(by_name["pair_index_out_of_range"])
    assert e["totals"][:2] == [2, 1]
    e = lc.restate(by_name["pair_of_a_frame_with_itself"])
    assert e["totals"] == [2, 1, 0, 0]
    c = by_name["inlier_zero_keeps_two_tracks_apart"]
    assert lc.restate(c, True)["totals"][:2] == [4, 2] and lc.restate(c, False)["totals"][:2] == [4, 1]
    e = lc.restate(by_name["cycle"])
    assert e["totals"] == [3, 1, 0, 0]
    e = lc.restate(by_name["same_edge_twice_and_both_directions"])
    assert e["totals"] == [2, 1, 0, 0]


def test_larger_cases_reach_what_they_are_for():
    e = lc.restate(lc.chain())
    assert e["totals"] == [1200, 4, 0, 0] and e["point_len"][:4] == [300] * 4
    e = lc.restate(lc.hub())
    assert e["totals"] == [257, 1, 0, 0] and e["node_point"].count(lr.SHORT) == 257
    e = lc.restate(lc.hub(True))
    assert e["totals"] == [0, 0, 1, 0] and e["node_point"].count(lr.CONFLICT) == 258
    for e in lc.random_case()[1:]:  # the GPU test cannot pass vacuously
        print("random case: totals", e["totals"])
        assert e["totals"][2] >= 1 and e["totals"][1] >= 60


def test_properties_of_every_output():
    for c in _all_cases():
        for mv in (2, 3):
            e = lc.restate(c, True, mv)
            N, cap = c["n_frames"] * c["cap"], c["cap"]
            n_obs, n_points = e["totals"][:2]
            for k in ("node_point", "obs_cam", "obs_point", "obs_node", "obs_xy"):
                assert len(e[k]) == N, (c["name"], k)
            assert len(e["point_len"]) == N // 2
            assert all(a < b for a, b in zip(e["obs_node"][:n_obs], e["obs_node"][1:n_obs])), c["name"]  # strictly ascending
            assert sum(e["point_len"]) == n_obs and all(v == 0 for v in e["point_len"][n_points:]), c["name"]
            assert e["obs_cam"][n_obs:] == [-1] * (N - n_obs) and e["obs_xy"][n_obs:] == [(0.0, 0.0)] * (N - n_obs)
            frames = {}
            for k in range(n_obs):
                assert e["obs_cam"][k] == e["obs_node"][k] // cap and e["node_point"][e["obs_node"][k]] == e["obs_point"][k]
                frames.setdefault(e["obs_point"][k], []).append(e["obs_cam"][k])
            assert sorted(frames) == list(range(n_points))
            for p, fs in frames.items():  # every track: pairwise distinct frames, at least min_views of them
                assert len(set(fs)) == len(fs) == e["point_len"][p] >= mv, (c["name"], p)


def test_wide_case_reaches_every_verdict_past_the_second_trip_of_the_flags_kernel():
    """tests/map_wide_cases.py: N + 1 > 1024 * 256, and a track, a counted SHORT component and a CONFLICT each have their label --
    where link_flags counts them -- past node 262144; so have observations."""
    import map_wide_cases as wide
    c = wide.link_case()
    assert c["n_frames"] * c["cap"] + 1 > wide.SECOND_TRIP and set(np.flatnonzero(c["counts"])) == set(wide.LOW + wide.HIGH)
    for min_views in (2, 3):
        e = wide.link_restated(True, min_views)
        assert e["totals"][1] >= 2 and e["totals"][2] == 2 and e["totals"][3] == (16 if min_views == 3 else 0)
        high = {label: nodes for label, nodes in e["components"].items() if label >= wide.SECOND_TRIP}
        codes = {label: e["node_point"][label] for label in high}
        assert any(v >= 0 for v in codes.values()) and any(v == lr.CONFLICT for v in codes.values())
        assert any(v == lr.SHORT and len(high[label]) >= 2 for label, v in codes.items()) == (min_views == 3)
        n_obs = e["totals"][0]
        assert max(e["obs_node"][:n_obs]) > wide.SECOND_TRIP
    # the inlier byte 0 keeps row 12 of either group at two views
    assert wide.link_restated(False, 3)["totals"][3] == 14
