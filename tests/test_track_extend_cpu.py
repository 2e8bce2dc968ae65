"""What the inputs of tests/track_extend_cases.py reach, and the restatement tests/track_extend_restate.py against an independent
brute force (the (frame, point) sets enumerated, the components flood-filled) and, without a map and without claims, against
tests/track_link_restate.py.  No GPU: the last test only asks the library for the entry and hands it a NULL context.
tests/test_track_extend_gpu.py holds the device to the restatement."""
import ctypes as C

import numpy as np

import track_extend_cases as ec
import track_extend_restate as er
import track_link_cases as lc
import track_link_restate as lr


def _all_cases():
    return [ec.census(), ec.hub(), ec.hub(True), ec.chain(), ec.random_case()[0]] + ec.boundaries()


def _brute(c, use_inlier, min_views):
    """node_point and totals from arrays and loops that share nothing with the restatement."""
    F, cap, n_points = c["n_frames"], c["cap"], c["n_points"]
    N = F * cap
    cnt = np.clip(c["counts"].astype(np.int64), 0, cap)
    exists = (np.arange(N) % cap) < cnt[np.arange(N) // cap]
    mapped = exists & (c["node_point"] >= 0) & (c["node_point"] < n_points)
    claims = exists & ~mapped & (c["row_inlier"] != 0) & (c["row_point"] >= 0) & (c["row_point"] < n_points)
    out = np.full(N, er.NO_ROW, np.int64)
    out[mapped] = c["node_point"][mapped]
    adopted = rejected = 0
    for f in range(F):
        nodes = np.arange(f * cap, (f + 1) * cap)
        for p in range(n_points):
            holders = nodes[mapped[nodes] & (c["node_point"][nodes] == p)]
            wanting = nodes[claims[nodes] & (c["row_point"][nodes] == p)]
            if len(wanting) == 1 and len(holders) == 0:
                out[wanting] = p
                adopted += 1
            else:
                out[wanting] = er.REJECTED
                rejected += len(wanting)
    free = exists & ~mapped & ~claims
    adj = {int(n): set() for n in np.flatnonzero(free)}
    for k in range(len(c["pair_q"])):
        q, t = int(c["pair_q"][k]), int(c["pair_t"][k])
        if q == t or not (0 <= q < F and 0 <= t < F):
            continue
        for i in range(int(cnt[q])):
            j = int(c["idx1"][k, i])
            if (use_inlier and c["inlier"][k, i] == 0) or not 0 <= j < cnt[t]:
                continue
            a, b = q * cap + i, t * cap + j
            if a in adj and b in adj:
                adj[a].add(b)
                adj[b].add(a)
    seen, n_total, n_conflict, n_short = set(), n_points, 0, 0
    for start in sorted(adj):  # ascending: a component is met first at its smallest node
        if start in seen:
            continue
        comp, stack = {start}, [start]
        while stack:
            for nb in adj[stack.pop()]:
                if nb not in comp:
                    comp.add(nb)
                    stack.append(nb)
        seen |= comp
        frames = [n // cap for n in comp]
        if len(set(frames)) < len(frames):
            code, n_conflict = er.CONFLICT, n_conflict + 1
        elif len(comp) < min_views:
            code, n_short = er.SHORT, n_short + (len(comp) >= 2)
        else:
            code, n_total = n_total, n_total + 1
        out[list(comp)] = code
    return out.tolist(), [int((out >= 0).sum()), n_total, adopted, rejected, n_conflict, n_short]


def test_restatement_equals_the_brute_force():
    for c in [ec.census(), ec.random_case()[0]] + ec.boundaries():
        for use_inlier in (True, False):
            for mv in (2, 3):
                e = ec.restate(c, use_inlier, min_views=mv)
                node_point, totals = _brute(c, use_inlier, mv)
                assert e["totals"] == totals, (c["name"], use_inlier, mv, e["totals"], totals)
                assert e["node_point"] == node_point, (c["name"], use_inlier, mv)


def test_census_reaches_every_code_and_every_total():
    c = ec.census()
    cap = c["cap"]
    node = lambda f, i: f * cap + i
    e3, e2 = ec.restate(c), ec.restate(c, min_views=2)
    assert c["min_views"] == 3
    n_obs, n_total, n_adopted, n_rejected, n_conflict, n_short = e3["totals"]
    assert n_obs > 0 and n_total == c["n_points"] + 1 and n_adopted == 4 and n_rejected == 8 and n_conflict == 1 and n_short == 1
    assert e2["totals"][1] == c["n_points"] + 2 and e2["totals"][5] == 0
    assert {min(v, 0) for v in e3["node_point"]} == {0, er.SHORT, er.CONFLICT, er.NO_ROW, er.REJECTED}
    np3 = e3["node_point"]
    assert e3["state"][node(0, 0)] == (er.MAPPED, 0) and np3[node(0, 0)] == 0                        # a MAPPED node (its claim is not read)
    assert [np3[node(f, 0)] for f in (3, 4, 5)] == [0, 0, 0] and np3[node(4, 6)] == 2                # ADOPTED, three frames one point
    assert np3[node(3, 1)] == er.REJECTED and np3[node(3, 7)] == 2                                   # against a MAPPED node of the frame
    assert [np3[node(4, i)] for i in (1, 2)] == [er.REJECTED] * 2                                    # two claimants in one frame
    assert [np3[node(4, i)] for i in (3, 4, 5)] == [er.REJECTED] * 3                                 # three claimants in one frame
    assert e3["state"][node(3, 2)] == (er.FREE, None) and np3[node(3, 2)] == c["n_points"]           # row_inlier 0: FREE, in the new track
    assert [np3[node(f, i)] for f, i in ((3, 2), (4, 7), (5, 3))] == [c["n_points"]] * 3             # the new TRACK
    assert all(e3["state"][node(3, i)] == (er.FREE, None) for i in (3, 4, 5))                        # claims -1, n_points, -4
    assert all(e3["state"][node(0, i)] == (er.FREE, None) for i in (4, 5, 6))                        # node_point_in < 0, == n_points, INT32_MAX
    assert np3[node(3, 3)] == np3[node(1, 4)] == er.SHORT and e2["node_point"][node(3, 3)] == c["n_points"]  # FREE-MAPPED edge ignored
    assert np3[node(5, 4)] == er.SHORT and e2["node_point"][node(5, 4)] == er.SHORT                  # FREE-ADOPTED, FREE-REJECTED ignored
    assert [np3[node(f, i)] for f, i in ((2, 5), (3, 4), (3, 5))] == [er.CONFLICT] * 3               # CONFLICT
    assert np3[node(5, 6)] == np3[node(5, 7)] == er.NO_ROW                                           # NO_ROW, though they "claim"
    assert e3["point_len"][:c["n_points"] + 1] == [6, 2, 4, 2, 0, 3]                                 # point 4 ends with nothing
    assert e3["point_grew"][:c["n_points"]] == [1, 0, 1, 0, 0] and e3["point_new"][:c["n_points"] + 2] == [0] * 5 + [1, 0]
    without = ec.restate(c, use_inlier=False, min_views=2)
    assert without["node_point"][node(0, 3)] >= c["n_points"] and e2["node_point"][node(0, 3)] == er.SHORT  # the inlier byte 0


def test_larger_cases_reach_what_they_are_for():
    e = ec.restate(ec.hub())
    assert e["totals"] == [257 + 257, 4, 256, 0, 0, 0] and e["point_len"][:4] == [0, 257, 0, 257] and e["point_grew"][:3] == [0, 1, 0]
    e = ec.restate(ec.hub(True))
    assert e["totals"] == [257 + 257, 4, 255, 1, 0, 0] and e["point_len"][1] == 257 and e["node_point"][128 * 4] == er.REJECTED
    e = ec.restate(ec.chain())
    assert e["totals"] == [66 + 64 + 66, 4, 64, 0, 0, 0] and e["point_len"][:4] == [66, 0, 66, 64]
    assert e["node_point"][2] == 2 and e["node_point"][2 * 4 + 1] == 3  # ascending label: (0, 2) is node 2, (2, 1) is node 9
    c, with_inlier, without = ec.random_case()
    for e in (with_inlier, without):  # the GPU test cannot pass vacuously
        print("random growth: map points", c["n_points"], "totals", e["totals"])
        assert c["n_points"] >= 40 and e["totals"][1] - c["n_points"] >= 5 and min(e["totals"][2:5]) >= 1
    for c in ec.boundaries():
        e = ec.restate(c)
        N = c["n_frames"] * c["cap"]
        assert N in (512, 513) and min(e["totals"][2:5]) >= 1 and e["totals"][1] > c["n_points"]
        assert e["obs_node"][0] == 0 and e["obs_node"][e["totals"][0] - 1] == (c["n_frames"] - 1) * c["cap"] + int(c["counts"][-1]) - 1


def test_without_a_map_and_claims_it_is_the_link():
    for c in lc.census() + [lc.random_case()[0]]:
        for use_inlier in (True, False):
            args = (c["kps"][..., :2], c["counts"].tolist(), c["n_frames"], c["cap"], c["pair_q"].tolist(), c["pair_t"].tolist(),
                    c["idx1"].reshape(-1).tolist(), c["inlier"].reshape(-1).tolist() if use_inlier else None)
            want = lr.link(*args, lc.INTRINSICS, c["min_views"])
            N = c["n_frames"] * c["cap"]
            for node_point_in, n_points in ((None, 0), ([0] * N, 0), (None, 7)):
                got = er.extend(*args, node_point_in, n_points, None, None, lc.INTRINSICS, c["min_views"])
                shift = lambda v: [x + n_points if x >= 0 else x for x in v]
                assert got["node_point"] == shift(want["node_point"]) and got["obs_point"] == shift(want["obs_point"]), c["name"]
                for k in ("obs_cam", "obs_xy", "obs_node"):
                    assert got[k] == want[k], (c["name"], k)
                assert got["point_len"][n_points:n_points + N // 2] == want["point_len"] and not any(got["point_len"][:n_points])
                assert [got["totals"][i] for i in (0, 1, 4, 5)] == [want["totals"][0], want["totals"][1] + n_points] + want["totals"][2:]
                assert got["totals"][2:4] == [0, 0] and not any(got["point_grew"])


def test_properties_of_every_output():
    for c in _all_cases():
        for mv in (2, 3):
            e = ec.restate(c, min_views=mv)
            N, cap, n_points = c["n_frames"] * c["cap"], c["cap"], c["n_points"]
            PC = n_points + N // 2
            n_obs, n_total = e["totals"][:2]
            for k in ("node_point", "obs_cam", "obs_point", "obs_node", "obs_xy"):
                assert len(e[k]) == N, (c["name"], k)
            assert all(len(e[k]) == PC for k in ("point_len", "point_new", "point_grew")) and n_points <= n_total <= PC
            assert all(a < b for a, b in zip(e["obs_node"][:n_obs], e["obs_node"][1:n_obs])), c["name"]  # ascending in node id
            assert e["obs_cam"][n_obs:] == [-1] * (N - n_obs) and e["obs_xy"][n_obs:] == [(0.0, 0.0)] * (N - n_obs)
            assert sum(e["point_len"]) == n_obs and not any(e["point_len"][n_total:]), c["name"]
            assert e["point_new"] == [0] * n_points + [1] * (n_total - n_points) + [0] * (PC - n_total)
            mapped = [n for n in range(N) if e["state"].get(n, (None,))[0] == er.MAPPED]
            assert all(e["node_point"][n] == c["node_point"][n] for n in mapped), c["name"]                # old ids untouched
            frames = {}
            for k in range(n_obs):
                assert e["obs_cam"][k] == e["obs_node"][k] // cap and e["node_point"][e["obs_node"][k]] == e["obs_point"][k]
                frames.setdefault(e["obs_point"][k], []).append(e["obs_cam"][k])
            assert sorted(p for p in frames if p >= n_points) == list(range(n_points, n_total))           # new ids contiguous from n_points
            for p, fs in frames.items():
                assert len(fs) == e["point_len"][p]
                if p >= n_points:  # no new track has two nodes of one frame
                    assert len(set(fs)) == len(fs) >= mv, (c["name"], p)
            pairs = [(n // cap, p) for n, p in e["adopted"].items()]
            assert len(set(pairs)) == len(pairs), c["name"]                                                # no ADOPTED (frame, point) twice
            assert all(e["point_grew"][p] == (1 if p in set(e["adopted"].values()) else 0) for p in range(PC))


def test_library_exports_the_entry_and_rejects_a_null_context():
    from gslam_amd import hip
    assert "gh_extend_tracks_dev" in hip.SIGNATURES and "gh_extend_tracks_dev" not in hip.MISSING
    fn = hip.lib.gh_extend_tracks_dev
    dummy = C.c_void_p(256)  # (never dereferenced: the context is checked first)
    args = [None, dummy, dummy, 1, 1, None, None, 0, None, None, None, 0, None, None] + [C.c_double(v) for v in lc.INTRINSICS] + [2] + [dummy] * 9
    assert fn(*args) == 1  # GH_ERR_ARG


def test_wide_case_reaches_every_verdict_past_the_second_trip_of_the_flags_kernel():
    """tests/map_wide_cases.py: N + 1 > 1024 * 256; an ADOPTED and a REJECTED claimant, and the labels of a new track, of a counted
    SHORT component and of a CONFLICT -- where ext_flags counts them -- all lie past node 262144; so do observations."""
    import map_wide_cases as wide
    c = wide.extend_case()
    assert c["n_frames"] * c["cap"] + 1 > wide.SECOND_TRIP and c["min_views"] == 3
    e = wide.extend_restated()
    n_obs, n_total, n_adopted, n_rejected, n_conflict, n_short = e["totals"]
    assert n_total > c["n_points"] and n_adopted == 2 and n_rejected == 5 and n_conflict == 2 and n_short == 16
    assert any(n > wide.SECOND_TRIP for n in e["adopted"]) and sum(n > wide.SECOND_TRIP for n in e["rejected"]) == 3
    high = {label: nodes for label, nodes in e["components"].items() if label >= wide.SECOND_TRIP}
    codes = {label: e["node_point"][label] for label in high}
    assert any(v >= c["n_points"] for v in codes.values()) and any(v == er.CONFLICT for v in codes.values())
    assert any(v == er.SHORT and len(high[label]) >= 2 for label, v in codes.items())
    assert max(e["obs_node"][:n_obs]) > wide.SECOND_TRIP
    assert wide.extend_restated(True, True, True, 2)["totals"][5] == 0
