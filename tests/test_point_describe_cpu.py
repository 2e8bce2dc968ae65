"""No GPU: tests/point_describe_restate.py against an independent numpy brute force (np.sort of the distance matrix, the mean of
the unit rays), and a census of tests/point_describe_cases.py: the cases reach what their docstrings claim, with the counts
printed."""
import math

import numpy as np

import point_describe_cases as pc
import point_describe_restate as pr


def _brute(c):
    """numpy on the case's arrays -> per point (state, L, chosen observation, reference observation, normal, dist)."""
    F, cap, P = c["n_frames"], c["cap"], c["n_points"]
    N = F * cap
    point, node, cam = c["obs_point"].astype(np.int64), c["obs_node"].astype(np.int64), c["obs_cam"].astype(np.int64)
    ok = (c["obs_use"] != 0) & (point >= 0) & (point < P) & (node >= 0) & (node < N)
    safe = np.where(ok, node, 0)
    ok &= (safe % cap < np.clip(c["counts"], 0, cap)[safe // cap]) & (cam == safe // cap)
    bits = np.unpackbits(c["desc"].reshape(N, 32), axis=1).astype(np.int32)
    octave = c["kps"][..., 5].copy().view(np.int32).reshape(-1)
    pw = float(c["scale_factor"]) ** np.arange(c["n_levels"])
    out = {}
    for p in range(P):
        if c["select"][p] == 0:
            out[p] = (pr.SKIPPED,)
            continue
        if c["status"][p] != 0:
            out[p] = (pr.NOT_OK,)
            continue
        ks = np.flatnonzero(ok & (point == p))
        L = len(ks)
        if L == 0:
            out[p] = (pr.EMPTY,)
            continue
        M = min(L, c["max_views"])
        cand = ks if L <= c["max_views"] else ks[(np.arange(M, dtype=np.int64) * L) // M]
        b = bits[node[cand]]
        D = (b[:, None, :] != b[None, :, :]).sum(2)
        med = np.sort(D, axis=1)[:, (M - 1) // 2]
        best = int(np.argmin(med))  # the first minimum
        v = c["xyz"][p] - c["poses"][node[ks] // cap, 4:]
        with np.errstate(all="ignore"):
            r = np.linalg.norm(v, axis=1)
            normal = (v / r[:, None]).mean(0)
        level = int(np.clip(octave[node[ks[0]]], 0, c["n_levels"] - 1))
        hi = r[0] * pw[level]
        out[p] = (pr.OK, L, int(cand[best]), int(ks[0]), normal, (hi / pw[-1], hi), int(med[best]))
    return out


def test_restatement_equals_a_numpy_brute_force():
    for c in pc.cases():
        e = pc.restate(c)
        b = _brute(c)
        P = c["n_points"]
        assert len(e["point_state"]) == P
        n = [0, 0, 0, 0]
        for p in range(P):
            assert e["point_state"][p] == b[p][0], (c["name"], p)
            n[b[p][0]] += 1
            if b[p][0] != pr.OK:
                continue
            _, L, chosen, ref, normal, dist, med = b[p]
            assert e["point_views"][p] == L and e["point_obs"][p] == [chosen, ref] and e["med"][p] == med, (c["name"], p)
            want = c["desc"].reshape(-1, 32)[c["obs_node"][chosen]].tobytes()
            assert int(e["point_desc"][p]).to_bytes(32, "little") == want, (c["name"], p)
            got = np.array(e["point_normal"][p])
            assert np.array_equal(np.isnan(got), np.isnan(normal)), (c["name"], p)
            if not np.isnan(got).any():
                assert np.allclose(got, normal, rtol=0, atol=1e-13), (c["name"], p)
            assert np.allclose(e["point_dist"][p], dist, rtol=1e-13, atol=0), (c["name"], p)
        assert e["totals"][:3] == [n[pr.OK], n[pr.EMPTY], n[pr.NOT_OK]], c["name"]
        assert e["totals"][3] == sum(1 for p in range(P) if b[p][0] == pr.OK and b[p][1] > c["max_views"]), c["name"]


def test_skipped_points_keep_what_went_in():
    c = pc.soup(64)
    P = c["n_points"]
    prev = dict(point_desc=[7] * P, point_obs=[[5, 6]] * P, point_views=[9] * P, point_normal=[[1.0, 2.0, 3.0]] * P,
                point_dist=[[4.0, 5.0]] * P)
    e = pr.describe(**pc.as_lists(c), prev=prev)
    base = pc.restate(c)
    skipped = [p for p in range(P) if e["point_state"][p] == pr.SKIPPED]
    assert len(skipped) == 2
    for p in range(P):
        for k in ("point_desc", "point_obs", "point_views", "point_normal", "point_dist"):
            assert e[k][p] == (prev[k][p] if p in skipped else base[k][p]), (k, p)


def _other_rules(cand_desc):
    """The candidate that rules near the contract's would choose -> dict rule -> candidate."""
    M = len(cand_desc)
    D = [[bin(a ^ b).count("1") for b in cand_desc] for a in cand_desc]
    first_min = lambda v: min(range(M), key=lambda c: (v[c], c))
    out = {"upper": first_min([sorted(r)[M // 2] for r in D]),
           "mean": first_min([sum(r) for r in D]),
           "last": max(range(M), key=lambda c: (-sorted(D[c])[(M - 1) // 2], c))}
    if M > 1:
        out["no_self"] = first_min([sorted(r[:a] + r[a + 1:])[(M - 2) // 2] for a, r in enumerate(D)])
    return out


def test_census():
    lengths, states, ref_octaves, rounding, n_ok = set(), set(), set(), 0, 0
    differ = {}
    for c in pc.cases():
        e = pc.restate(c)
        a = pc.as_lists(c)
        for p in range(c["n_points"]):
            states.add(e["point_state"][p])
            if e["point_state"][p] != pr.OK:
                continue
            track = e["tracks"][p]
            L = len(track)
            lengths.add((L, c["max_views"]))
            ref_octaves.add(a["kps_octave"][a["obs_node"][track[0]]])
            # rank is by observation index: the track ascends although the arrays are shuffled
            assert track == sorted(track)
            cand = pr.candidates(track, c["max_views"])
            assert cand == sorted(set(cand)) and len(cand) == min(L, c["max_views"])  # strictly increasing
            if c["name"].startswith("soup") and len(cand) > 1:
                chosen = cand.index(e["point_obs"][p][0])
                for rule, other in _other_rules([a["desc"][a["obs_node"][k]] for k in cand]).items():
                    d = differ.setdefault((rule, c["max_views"]), [0, 0])
                    d[0] += other != chosen
                    d[1] += 1
            if c["name"] == "identical":
                assert e["point_obs"][p][0] == track[0] and e["med"][p] == 0
            # another addition order: one running sum in live order
            if L >= 3:
                n_ok += 1
                s = [0.0, 0.0, 0.0]
                for k in track:
                    u, _ = pr.unit_ray(a["xyz"][p], a["poses"][a["obs_node"][k] // c["cap"]][4:7])
                    s = [s[i] + u[i] for i in range(3)]
                seq = [pr.canonical(pr.div(s[i], float(L))) for i in range(3)]
                rounding += np.array(seq).tobytes() != np.array(e["point_normal"][p]).tobytes()
    print("lengths (L, max_views):", sorted(lengths))
    for L in pc.SOUP_LENGTHS:
        for mv in pc.SOUP_MAX_VIEWS:
            assert (L, mv) in lengths, (L, mv)
    assert (4096, 64) in lengths
    assert states == {pr.OK, pr.EMPTY, pr.NOT_OK, pr.SKIPPED}
    assert {-3, 0, 7, 40} <= ref_octaves, ref_octaves
    print("tracks of three or more whose direction changes bits under one running sum: %d of %d" % (rounding, n_ok))
    assert rounding >= n_ok // 4
    for key in sorted(differ):
        print("rule %-7s max_views %2d: another candidate in %d of %d tracks" % (key + tuple(differ[key])))
    for rule in ("upper", "mean", "last", "no_self"):
        assert sum(differ[(rule, mv)][0] for mv in pc.SOUP_MAX_VIEWS if (rule, mv) in differ) > 0, rule
    assert differ[("last", 64)][0] > 0 and differ[("upper", 64)][0] > 0 and differ[("mean", 9)][0] > 0

    # the soup hits both sides of both kernel boundaries: M <= 8 and M > 8, L <= max_views and L > max_views
    e = pc.restate(pc.soup(64))
    assert e["totals"][3] == 8  # 65, 127, 128, 200 twice (the track of 70 is NOT_OK)
    views = sorted(v for v in e["point_views"] if v)
    assert {8, 9, 64, 65} <= set(views)

    # every way an observation is dropped
    c = pc.drops()
    e = pc.restate(c)
    kept = {k for t in e["tracks"] for k in t}
    why = c["why"]
    for reason in ("point", "node", "count", "cam", "masked"):
        ks = np.flatnonzero(why == reason)
        assert len(ks) >= 1 and not (set(ks.tolist()) & kept), reason
    assert set(np.flatnonzero(why == "kept").tolist()) <= kept
    assert (c["obs_use"] == 0).sum() >= 2 and (c["counts"] < 0).any() and (c["counts"] > c["cap"]).any()
    print("drops: %d observations, %d usable" % (len(why), len(kept)))

    # the point at a camera centre: NaN direction; as the reference also dist = 0
    c = pc.centre()
    e = pc.restate(c)
    nan_points = [p for p in range(c["n_points"]) if e["point_state"][p] == pr.OK and any(math.isnan(v) for v in e["point_normal"][p])]
    assert sorted(nan_points) == sorted(int(v) for v in c["track_ids"][:3])
    assert e["point_dist"][int(c["track_ids"][0])] == [0.0, 0.0]
    assert all(np.array(e["point_normal"][p]).tobytes() == np.array([pr.NAN] * 3).tobytes() for p in nan_points)

    c = pc.long_track()
    e = pc.restate(c)
    assert max(e["point_views"]) == 4096 and sum(1 for v in e["point_views"] if 2 <= v <= 6) == 500 and e["totals"][3] == 1
    assert len(c["obs_point"]) < 8000
