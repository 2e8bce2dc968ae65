"""What the inputs of tests/track_merge_cases.py reach, and the restatement tests/track_merge_restate.py against an independent
brute force (an explicit adjacency over integer elements, flood-filled, numpy for the classes and the gate) and, with every
node its own point, against tests/track_link_restate.py.  No GPU: the last test only asks the library for the entry and hands
it a NULL context.  tests/test_track_merge_gpu.py holds the device to the restatement."""
import ctypes as C
import itertools

import numpy as np

import track_link_cases as lc
import track_link_restate as lr
import track_merge_cases as mc
import track_merge_restate as mr

VARIANTS = list(itertools.product((True, False), (True, False), (True, False), (1, 0)))  # inlier, status, gate, bridge


def _all_cases():
    return [mc.census(), mc.fused(), mc.hub(), mc.hub(True), mc.chain(), mc.random_case()[0]] + mc.boundaries()


def _brute(c, use_inlier, use_status, use_gate, bridge):
    """remap, state and totals from arrays and loops that share nothing with the restatement."""
    F, cap, P = c["n_frames"], c["cap"], c["n_points"]
    N = F * cap
    cnt = np.clip(c["counts"].astype(np.int64), 0, cap)
    exists = (np.arange(N) % cap) < cnt[np.arange(N) // cap]
    v = c["node_point"].astype(np.int64)
    valid = exists & (v >= 0) & (v < P)
    ok = np.ones(P, bool) if not use_status else c["status"] == 0
    holder = valid.copy()
    holder[valid] = ok[v[valid]]
    elem = np.full(N, -1, np.int64)
    elem[holder] = v[holder]
    if bridge:
        free = exists & ~valid
        elem[free] = P + np.flatnonzero(free)
    adj = {}
    for k in range(len(c["pair_q"])):
        q, t = int(c["pair_q"][k]), int(c["pair_t"][k])
        if q == t or not (0 <= q < F and 0 <= t < F):
            continue
        for i in range(int(cnt[q])):
            j = int(c["idx1"][k, i])
            if (use_inlier and c["inlier"][k, i] == 0) or not 0 <= j < cnt[t]:
                continue
            a, b = int(elem[q * cap + i]), int(elem[t * cap + j])
            if a >= 0 and b >= 0 and a != b:
                adj.setdefault(a, set()).add(b)
                adj.setdefault(b, set()).add(a)
    remap, state, totals, seen = np.arange(P), np.zeros(P, np.int64), [0] * 6, set()
    for start in range(P):  # ascending: a component is met first at its smallest point
        if start in seen or start not in adj:
            continue
        comp, stack = {start}, [start]
        while stack:
            for nb in adj[stack.pop()]:
                if nb not in comp:
                    comp.add(nb)
                    stack.append(nb)
        seen |= comp
        pts = np.array(sorted(e for e in comp if e < P))
        if len(pts) < 2:
            continue
        frames = np.flatnonzero(holder & np.isin(v, pts)) // cap
        with np.errstate(invalid="ignore"):
            d = c["xyz"][pts] - c["xyz"][start]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            near = bool((d2 <= c["max_dist"] * c["max_dist"]).all())
        if len(np.unique(frames)) != len(frames):
            state[pts], totals[2], totals[5] = mr.CONFLICT, totals[2] + 1, totals[5] + len(pts)
        elif use_gate and not near:
            state[pts], totals[3], totals[5] = mr.FAR, totals[3] + 1, totals[5] + len(pts)
        else:
            state[pts], remap[pts] = mr.ABSORBED, start
            state[start] = mr.SURVIVOR
            totals[0], totals[1] = totals[0] + 1, totals[1] + len(pts) - 1
    out = np.where((v >= 0) & (v < P), remap[np.clip(v, 0, max(P - 1, 0))], v)
    totals[4] = int((exists & (out != v)).sum())
    point_len = np.bincount(out[exists & (out >= 0) & (out < P)], minlength=P)
    return dict(point_remap=remap.tolist(), point_state=state.tolist(), node_point=out.tolist(), point_len=point_len.tolist(), totals=totals)


def test_restatement_matches_the_brute_force():
    for c in _all_cases():
        for use_inlier, use_status, use_gate, bridge in VARIANTS if c["n_points"] < 100 else VARIANTS[:1] + VARIANTS[-1:]:
            e, b = mc.restate(c, use_inlier, use_status, use_gate, bridge), _brute(c, use_inlier, use_status, use_gate, bridge)
            for k in b:
                assert e[k] == b[k], (c["name"], use_inlier, use_status, use_gate, bridge, k)
            assert e["point_select"] == [1 if s == mr.SURVIVOR else 0 for s in e["point_state"]]


def test_census_reaches_every_state_and_every_total():
    c = mc.census()
    e = mc.restate(c)
    assert e["totals"] == [4, 5, 2, 3, 5, 10]
    assert e["verdict"] == {0: 1, 2: 1, 4: 1, 20: 1, 7: mr.CONFLICT, 9: mr.CONFLICT, 11: mr.FAR, 13: mr.FAR, 15: mr.FAR}
    assert set(e["point_state"]) == {mr.NONE, mr.SURVIVOR, mr.ABSORBED, mr.CONFLICT, mr.FAR}
    assert e["groups"][4] == [4, 5, 6] and e["point_remap"][5] == e["point_remap"][6] == 4
    # exactly max_dist merges, one ulp beyond does not
    assert mr.d2(c["xyz"][1], c["xyz"][0]) == c["max_dist"] ** 2 and e["point_state"][1] == mr.ABSORBED
    assert mr.d2(c["xyz"][14], c["xyz"][13]) == np.nextafter(25.0, 26.0) and e["point_state"][14] == mr.FAR
    # the unusable point 17 keeps 18 and 19 apart; the row (5,6) that does not exist is renamed and counts in nothing
    assert [e["point_state"][p] for p in (17, 18, 19, 22, 23, 24, 25)] == [mr.NONE] * 7
    assert c["node_point"][5 * 8 + 6] == 1 and e["node_point"][5 * 8 + 6] == 0 and e["point_len"][:2] == [3, 0]
    assert e["node_point"][5 * 8 + 1] == -4 and e["node_point"][4 * 8 + 5] == c["n_points"] and e["node_point"][3 * 8 + 5] == mc.INT32_MAX
    # what each switch changes
    assert mc.restate(c, bridge=0)["totals"] == [2, 3, 2, 3, 3, 10]                  # B and J need their BRIDGE nodes
    assert mc.restate(c, use_inlier=False)["verdict"].get(22) == mr.SURVIVOR         # K
    assert mc.restate(c, use_status=False)["groups"].get(17) == [17, 18, 19]         # I
    assert mc.restate(c, use_gate=False)["totals"][2:4] == [2, 0]                    # F, G, H merge; D and E stay CONFLICT


def test_a_fused_multiply_add_would_change_a_verdict():
    a, b, max_dist, plain, fused = mc.fused_pair()
    assert plain == mr.d2(a, b) and fused == mc.fused_d2(a, b) and plain != fused
    assert (plain <= max_dist * max_dist) != (fused <= max_dist * max_dist)
    assert abs(plain - float(mc.exact_d2(a, b))) <= 2e-15 * plain
    e = mc.restate(mc.fused())
    assert e["totals"][0] + e["totals"][3] == 1 and (e["totals"][0] == 1) == (plain <= max_dist * max_dist)


def test_larger_cases_reach_what_they_were_built_for():
    assert mc.restate(mc.hub())["totals"] == [1, 256, 0, 0, 256, 0] and mc.restate(mc.hub())["point_len"][0] == 257
    assert mc.restate(mc.hub(True))["totals"] == [0, 0, 1, 0, 0, 257]
    e = mc.restate(mc.chain())
    assert e["totals"] == [1, 299, 0, 0, 598, 0] and e["point_len"] == [600] + [0] * 299
    for order in ("reversed", "shuffled"):
        assert mc.restate(mc.reorder(mc.chain(), order, seed=3))["point_remap"] == e["point_remap"]
    c, e = mc.random_case()
    print("random_split totals", e["totals"])
    assert e["totals"][0] >= 10 and e["totals"][2] >= 2 and e["totals"][3] >= 2  # the GPU test does not pass vacuously
    for c in mc.boundaries():
        e = mc.restate(c)
        assert min(e["totals"][:4]) >= 1, (c["name"], e["totals"])
    a, b = mc.boundaries()
    assert (a["n_frames"] * a["cap"], a["n_points"], b["n_frames"] * b["cap"], b["n_points"]) == (512, 257, 513, 256)


def test_every_node_its_own_point_gives_the_tracks_of_the_link():
    """n_points = N, node n holds point n, no gate: MERGED groups are the link's TRACKs, CONFLICT groups its CONFLICT
    components, the labels are the smallest nodes."""
    for c in lc.census() + [lc.random_case()[0], lc.chain("shuffled", seed=3), lc.hub(), lc.hub(True)]:
        N, cap = c["n_frames"] * c["cap"], c["cap"]
        for use_inlier in (True, False):
            want = lc.restate(c, use_inlier, 2)
            got = mr.merge(c["counts"].tolist(), c["n_frames"], cap, c["pair_q"].tolist(), c["pair_t"].tolist(),
                           c["idx1"].reshape(-1).tolist(), c["inlier"].reshape(-1).tolist() if use_inlier else None, list(range(N)), N)
            assert [got["totals"][0], got["totals"][2]] == want["totals"][1:3], c["name"]
            comps = {l: nodes for l, nodes in want["components"].items() if len(nodes) >= 2}
            assert got["groups"] == comps, c["name"]
            for l, nodes in comps.items():
                conflict = want["node_point"][l] == lr.CONFLICT
                assert got["verdict"][l] == (mr.CONFLICT if conflict else mr.SURVIVOR)
                assert all(got["point_remap"][n] == (n if conflict else l) for n in nodes)


def test_properties_of_every_output():
    for c in _all_cases():
        for bridge in (1, 0):
            e = mc.restate(c, bridge=bridge)
            P, N, cap = c["n_points"], c["n_frames"] * c["cap"], c["cap"]
            remap = e["point_remap"]
            assert all(len(e[k]) == P for k in ("point_remap", "point_state", "point_select", "point_len")) and len(e["node_point"]) == N
            assert all(remap[remap[p]] == remap[p] <= p for p in range(P)), c["name"]          # idempotent, onto smaller-or-equal ids
            exists = mr.existing(c["counts"], c["n_frames"], cap)
            assert sum(e["point_len"]) == sum(1 for n in exists if 0 <= c["node_point"][n] < P), c["name"]
            assert all(e["point_len"][p] == 0 for p in range(P) if e["point_state"][p] == mr.ABSORBED)
            assert e["totals"][1] == e["point_state"].count(mr.ABSORBED) and e["totals"][0] == sum(e["point_select"])
            assert e["totals"][5] == e["point_state"].count(mr.CONFLICT) + e["point_state"].count(mr.FAR)
            # the observation list keeps its length and order
            assert [o >= 0 for o in e["obs_point"]] == [o >= 0 for o in c["obs_point"].tolist()]
            assert e["obs_point"] == mc.obs_of(np.array(e["node_point"]), c["counts"], cap, P).tolist()
            # a second call on the outputs merges nothing
            again = mr.merge(c["counts"].tolist(), c["n_frames"], cap, c["pair_q"].tolist(), c["pair_t"].tolist(),
                             c["idx1"].reshape(-1).tolist(), c["inlier"].reshape(-1).tolist(), e["node_point"], P, c["status"].tolist(),
                             [tuple(r) for r in c["xyz"].tolist()], c["max_dist"], bridge, e["obs_point"])
            assert again["totals"][:2] == [0, 0] and again["totals"][4] == 0 and again["node_point"] == e["node_point"], c["name"]
            assert again["point_len"] == e["point_len"] and again["totals"][2:4] == e["totals"][2:4]


def test_split_then_merge_returns_the_original_map():
    s = mc.scene_split()
    F, cap, P = s["n_frames"], s["cap"], s["n_points"]
    assert len(s["split"]) >= 8 and (s["node_point_split"] != s["node_point"]).sum() >= 2 * len(s["split"])
    e = mr.merge(s["counts"].tolist(), F, cap, s["map_q"].tolist(), s["map_t"].tolist(), s["map_idx1"].reshape(-1).tolist(), None,
                 s["node_point_split"].tolist(), P, None, None, 0.0, 1, s["obs_point_split"].tolist())
    assert e["node_point"] == s["node_point"].tolist() and e["obs_point"] == s["obs_point"].tolist()
    assert e["totals"] == [len(s["split"]), len(s["split"]), 0, 0, int((s["node_point_split"] != s["node_point"]).sum()), 0]
    assert sorted(p for p in range(P) if e["point_select"][p]) == sorted(s["split"].values())


def test_library_exports_the_entry_and_rejects_a_null_context():
    from gslam_amd import estimator, hip
    assert "gh_merge_points_dev" in hip.SIGNATURES and "gh_merge_points_dev" not in hip.MISSING
    assert (estimator.MERGE_NONE, estimator.MERGE_SURVIVOR, estimator.MERGE_ABSORBED, estimator.MERGE_CONFLICT, estimator.MERGE_FAR) == \
        (mr.NONE, mr.SURVIVOR, mr.ABSORBED, mr.CONFLICT, mr.FAR)
    dummy = C.c_void_p(256)  # (never dereferenced: the context is checked first)
    args = [None, dummy, 1, 1, None, None, 0, None, None, dummy, 1, None, None, C.c_double(0.0), 1, None] + [dummy] * 3 + [dummy, None] + \
        [dummy] * 2
    assert len(args) == len(hip.SIGNATURES["gh_merge_points_dev"][1])
    assert hip.lib.gh_merge_points_dev(*args) == 1  # GH_ERR_ARG
