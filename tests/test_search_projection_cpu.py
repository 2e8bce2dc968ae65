"""What the inputs of tests/search_projection_cases.py reach, without a GPU: the plain-Python restatement
(tests/search_projection_restate.py) against an independent numpy brute force -- all points x all keypoints of a frame, no grid,
whole-array arithmetic in the contract's order -- in every NULL-variant; a census that proves each case reaches what it claims
(printed: run with -s); and three near rules (a closed window, ORB-SLAM's logarithm for the level, the highest row on ties),
each of which must change an output, so that the cases can tell the rules apart."""
import collections

import numpy as np
import pytest

import search_projection_cases as sc
import search_projection_restate as sr

CASES = {c["name"]: c for c in sc.cases()}
CELL = 32  # gh_search_cell_pixels(); tests/test_search_projection_build.py checks that the library says the same


def _popcount(a):
    return np.unpackbits(a, axis=-1).sum(-1).astype(np.int64)


def brute(c, use_map=True, use_claims=True, use_status=True, use_select=True):
    """The contract over whole arrays -> row_point, row_inlier, row_dist, frame_totals, totals as host arrays."""
    F, cap, P = c["n_frames"], c["cap"], c["n_points"]
    N = F * cap
    prm = c["params"]
    fx, fy, cx, cy = c["intrinsics"]
    W, H = (float(v) for v in c["size"])
    x, y = c["kps"][..., 0].astype(np.float64), c["kps"][..., 1].astype(np.float64)
    octave = c["kps"][..., 5].copy().view(np.int32).astype(np.int64)
    rows = np.clip(c["counts"], 0, cap)
    exists = np.arange(cap)[None, :] < rows[:, None]
    taken = np.full((F, cap), -1, np.int64)
    if use_claims:
        rp = c["row_point"].reshape(F, cap).astype(np.int64)
        m = exists & (c["row_inlier"].reshape(F, cap) != 0) & (rp >= 0) & (rp < P)
        taken[m] = rp[m]
    if use_map:
        npt = c["node_point"].reshape(F, cap).astype(np.int64)
        m = exists & (npt >= 0) & (npt < P)
        taken[m] = npt[m]
    searchable = c["views"] > 0
    if use_select:
        searchable &= c["select"] != 0
    if use_status:
        searchable &= c["status"] == 0
    searched = np.flatnonzero(c["frame_search"] != 0)
    pw = np.ones(32)
    for l in range(1, 32):
        pw[l] = pw[l - 1] * prm["scale_factor"]
    ft = np.zeros((F, 10), np.int64)
    best_of = {}  # node -> (h, p)
    n_prop = np.zeros(F, np.int64)
    X, nrm = c["xyz"], c["normal"]
    min_dist, max_dist = c["dist"][:, 0], c["dist"][:, 1]
    ids = np.arange(P)
    with np.errstate(all="ignore"):
        for f in searched:
            q, t = c["poses"][f, :4], c["poses"][f, 4:]
            qc = np.array([-q[0], -q[1], -q[2], q[3]])
            d = X - t
            uvx, uvy, uvz = qc[1] * d[:, 2] - qc[2] * d[:, 1], qc[2] * d[:, 0] - qc[0] * d[:, 2], qc[0] * d[:, 1] - qc[1] * d[:, 0]
            uvx, uvy, uvz = uvx + uvx, uvy + uvy, uvz + uvz
            Xc0 = d[:, 0] + qc[3] * uvx + (qc[1] * uvz - qc[2] * uvy)
            Xc1 = d[:, 1] + qc[3] * uvy + (qc[2] * uvx - qc[0] * uvz)
            Xc2 = d[:, 2] + qc[3] * uvz + (qc[0] * uvy - qc[1] * uvx)
            iz = 1.0 / Xc2
            u, v = fx * (Xc0 * iz) + cx, fy * (Xc1 * iz) + cy
            dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            cosv = ((d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1]) + d[:, 2] * nrm[:, 2]) / dist
            level = (pw[None, :max(prm["n_levels"] - 1, 0)] * dist[:, None] < max_dist[:, None]).sum(1)
            radius = (prm["radius_scale"] * np.where(cosv > prm["near_cos"], prm["radius_near"], prm["radius_far"])) * pw[level]
            verdict = np.full(P, -1)
            left = searchable.copy()
            for code, fails in ((sr.HELD, np.isin(ids, taken[f][taken[f] >= 0])), (sr.BEHIND, ~(Xc2 > 1e-9)),
                                (sr.OUTSIDE, ~((0.0 <= u) & (u < W) & (0.0 <= v) & (v < H))),
                                (sr.RANGE, ~((dist >= prm["range_lo"] * min_dist) & (dist <= prm["range_hi"] * max_dist))),
                                (sr.ANGLE, ~(cosv >= prm["min_view_cos"]))):
                verdict[left & fails] = code
                left &= ~fails
            is_open = exists[f] & (taken[f] < 0)
            cand = (is_open[None, :] & (octave[f][None, :] >= level[:, None] - 1) & (octave[f][None, :] <= level[:, None]) &
                    (np.abs(x[f][None, :] - u[:, None]) < radius[:, None]) & (np.abs(y[f][None, :] - v[:, None]) < radius[:, None]))
            h = _popcount(c["desc"][f][None, :, :] ^ c["point_desc"][:, None, :])
            big = 1 << 40
            key = np.sort(np.where(cand, h * 65536 + np.arange(cap)[None, :], big), axis=1)
            key = np.concatenate([key, np.full((P, 2), big)], axis=1)  # (cap may be 1)
            for p in np.flatnonzero(left):
                k1, k2 = int(key[p, 0]), int(key[p, 1])
                if k1 == big:
                    verdict[p] = sr.NO_CANDIDATE
                    continue
                hb, ib = k1 >> 16, k1 & 0xFFFF
                hs, os_ = (k2 >> 16, int(octave[f, k2 & 0xFFFF])) if k2 != big else (256, -1)
                if hb > prm["max_hamming"]:
                    verdict[p] = sr.WEAK
                elif int(octave[f, ib]) == os_ and float(hb) > prm["nn_ratio"] * float(hs):
                    verdict[p] = sr.RATIO
                else:
                    n_prop[f] += 1
                    n = int(f) * cap + ib
                    best_of[n] = min(best_of.get(n, (hb, int(p))), (hb, int(p)))
            for code in range(8):
                ft[f, code] = int((verdict == code).sum())
    row_dist = np.full(N, 0xFFFF, np.uint16)
    if use_claims:
        row_point, row_inlier = c["row_point"].copy(), (c["row_inlier"] != 0).astype(np.uint8)
    else:
        row_point = np.where(exists.reshape(-1), sr.LOC_NO_POINT, sr.LOC_NO_ROW).astype(np.int32)
        row_inlier = np.zeros(N, np.uint8)
    for n, (hb, p) in best_of.items():
        row_point[n], row_inlier[n], row_dist[n] = p, 1, hb
        ft[n // cap, sr.WON] += 1
    ft[:, sr.LOST] = n_prop - ft[:, sr.WON]
    totals = list(ft.sum(0)) + [len(searched), int(searchable.sum()) if len(searched) else 0]
    return dict(row_point=row_point.astype(np.int32), row_inlier=row_inlier, row_dist=row_dist, frame_totals=ft.astype(np.int32),
                totals=np.array(totals, np.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_brute_force(name):
    c = CASES[name]
    for v in sc.VARIANTS:
        want = brute(c, *v)
        got = sc.as_arrays(sc.restate(c, *v), c["n_frames"])
        for k in sc.OUTPUTS:
            assert got[k].tobytes() == want[k].tobytes(), (name, v, k, np.flatnonzero(got[k].reshape(-1) != want[k].reshape(-1))[:10])


def _taken(c):
    F, cap, P = c["n_frames"], c["cap"], c["n_points"]
    exists = np.arange(cap)[None, :] < np.clip(c["counts"], 0, cap)[:, None]
    npt, rp = c["node_point"].reshape(F, cap), c["row_point"].reshape(F, cap)
    mapped = exists & (npt >= 0) & (npt < P)
    claimed = exists & ~mapped & (c["row_inlier"].reshape(F, cap) != 0) & (rp >= 0) & (rp < P)
    return exists, mapped, claimed


def test_census():
    """Each case reaches what search_projection_cases says it does."""
    total = collections.Counter()
    n_cand, span_x, span_y, over = collections.Counter(), set(), set(), set()
    taken_in_window = bad_map = bad_claim = wild_xy = wild_octave = equal_h = 0
    counts_seen = set()
    for c in CASES.values():
        e = sc.restate(c)
        F, cap, P = c["n_frames"], c["cap"], c["n_points"]
        per = collections.Counter(e["verdict"].values())
        total.update(per)
        print("%-15s %d frames x %d rows, %d points:" % (c["name"], F, cap, P), ", ".join("%s %d" % (sr.VERDICTS[k], per[k]) for k in sorted(per)))
        assert sum(per.values()) == e["totals"][10] * e["totals"][11] == sum(e["totals"][:10])
        exists, mapped, claimed = _taken(c)
        x, y = c["kps"][..., 0].astype(np.float64), c["kps"][..., 1].astype(np.float64)
        octave = c["kps"][..., 5].copy().view(np.int32)
        searched = c["frame_search"] != 0
        live = exists & searched[:, None]
        W, H = c["size"]
        wild_xy += int((live & ~mapped & ~claimed & ~((x >= 0) & (x < W) & (y >= 0) & (y < H))).sum())
        wild_octave += int((live & ((octave < 0) | (octave >= c["params"]["n_levels"]))).sum())
        npt, rp = c["node_point"].reshape(F, cap), c["row_point"].reshape(F, cap)
        bad_map += int((live & ((npt < -4) | (npt >= P))).sum())
        bad_claim += int((live & (c["row_inlier"].reshape(F, cap) != 0) & ((rp < -4) | (rp >= P))).sum())
        counts_seen |= {"zero" if v == 0 else "negative" if v < 0 else "above" if v > cap else "plain"
                        for v, s in zip(c["counts"].tolist(), searched) if s}
        proposals = collections.defaultdict(list)
        for (f, p), det in e["detail"].items():
            if "radius" not in det:
                continue
            u, v, r, level = det["u"], det["v"], det["radius"], det["level"]
            k = len(det["candidates"])
            n_cand[k if k <= 9 else (64 if k <= 64 else 65)] += 1
            if k:
                span_x.add(min(int((u + r) // CELL) - int((u - r) // CELL) + 1, 3))
                span_y.add(min(int((v + r) // CELL) - int((v - r) // CELL) + 1, 3))
                over |= {w for w, yes in (("left", u - r < 0), ("right", u + r >= W), ("top", v - r < 0), ("bottom", v + r >= H)) if yes}
            t = (mapped[f] | claimed[f]) & (octave[f] >= level - 1) & (octave[f] <= level) & (np.abs(x[f] - u) < r) & (np.abs(y[f] - v) < r)
            taken_in_window += int(t.sum())
            if e["verdict"][(f, p)] in (sr.WON, sr.LOST):
                proposals[f * cap + det["best"]].append((det["h_best"], p))
        for props in proposals.values():
            hs = sorted(props)
            if len(hs) > 1 and hs[0][0] == hs[1][0]:
                equal_h += 1
                n = [k for k, v in proposals.items() if v is props][0]
                assert e["row_point"][n] == hs[0][1] and e["verdict"][(n // cap, hs[1][1])] == sr.LOST
    print("all cases:", ", ".join("%s %d" % (sr.VERDICTS[k], total[k]) for k in sorted(total)))
    print("candidates per window:", dict(sorted(n_cand.items())), "(64: 10 .. 64, 65: more); cells crossed in x", sorted(span_x), "in y",
          sorted(span_y), "; windows over the borders:", sorted(over))
    print("TAKEN nodes that lie in a window %d; out-of-range map entries %d, claim values %d; open keypoints outside the image or not "
          "numbers %d; octaves outside the pyramid %d; nodes with two proposals at one distance %d; counts %s" %
          (taken_in_window, bad_map, bad_claim, wild_xy, wild_octave, equal_h, sorted(counts_seen)))
    assert all(total[k] > 0 for k in range(10)), total
    assert all(n_cand[k] > 0 for k in (0, 1, 8, 9, 65)), n_cand
    assert span_x == {1, 2, 3} and span_y == {1, 2, 3} and over == {"left", "right", "top", "bottom"}
    assert taken_in_window > 0 and bad_map > 0 and bad_claim > 0 and wild_xy > 10 and wild_octave > 0 and equal_h > 0
    assert counts_seen == {"zero", "negative", "above", "plain"}
    assert {c["params"]["n_levels"] for c in CASES.values()} >= {1, 8, 32}
    for c in CASES.values():  # both ends of the pyramid still match something
        if c["params"]["n_levels"] in (1, 32):
            assert sc.restate(c)["totals"][sr.WON] > 0, c["name"]


def _pow(prm, k):
    return sr.pow_table(prm["scale_factor"])[k]


def test_census_of_the_edges():
    c = sc.edges()
    e, tag = sc.restate(c), c["tag"]
    V, D = e["verdict"], e["detail"]
    prm = c["params"]
    for name, radius in (("near", 2.5), ("far", 4.0)):
        p = tag[name]
        det = D[(0, p)]
        assert det["radius"] == radius and det["level"] == 0 and (det["cos"] > prm["near_cos"]) == (name == "near")
        for k in range(4):
            on, inside = tag["%s_on_%d" % (name, k)][1], tag["%s_in_%d" % (name, k)][1]
            x_on, y_on = (float(c["kps"][0, on, j]) for j in (0, 1))
            x_in, y_in = (float(c["kps"][0, inside, j]) for j in (0, 1))
            assert max(abs(x_on - det["u"]), abs(y_on - det["v"])) == radius and on not in det["candidates"]       # exactly on it
            assert radius - max(abs(x_in - det["u"]), abs(y_in - det["v"])) < 1e-4 and inside in det["candidates"]  # one float inside
        assert V[(0, p)] == sr.WON
    cos = [D[(0, tag["cos_%d" % k][0])].get("cos") for k in range(5)]
    assert cos[0] > prm["near_cos"] > cos[1] and cos[2] > prm["min_view_cos"] > cos[3] > cos[4]
    assert [V[(0, tag["cos_%d" % k][0])] for k in range(5)] == [sr.NO_CANDIDATE, sr.WON, sr.WON, sr.ANGLE, sr.ANGLE]
    assert [V[(0, p)] == sr.BEHIND for p in tag["depth"]] == [True, False, True, True]
    assert [V[(0, p)] == sr.OUTSIDE for p in tag["border"]] == [False, True] * 4
    u = D[(0, tag["last_u"])]["u"]
    assert u < 640.0 and 640.0 - u < 1e-9 and V[(0, tag["last_u"])] != sr.OUTSIDE and V[(0, tag["first_out_u"])] == sr.OUTSIDE
    assert [V[(0, tag[k])] == sr.RANGE for k in ("range_hi_0", "range_hi_1", "range_lo_0", "range_lo_1")] == [False, True, False, True]
    assert V[(3, tag["centre"])] == sr.BEHIND and c["xyz"][tag["centre"]].tolist() == c["poses"][3, 4:].tolist()
    assert all(V[(f, p)] == sr.BEHIND for f in (1, 2) for p in range(c["n_points"]) if (f, p) in V)  # the poses with a NaN
    assert not any((0, p) in V for p in tag["not_searchable"])
    assert all(V[(4, p)] not in (sr.HELD, sr.WON, sr.LOST, sr.WEAK, sr.RATIO) for p in range(c["n_points"]) if (4, p) in V)  # no rows
    assert not any(f == 5 for f, _ in V)
    want = [sr.WON, sr.WEAK, sr.WON, sr.RATIO, sr.WON, sr.WON]
    assert [V[(0, tag["match_%d" % k][0])] for k in range(6)] == want
    assert [D[(0, tag["match_%d" % k][0])]["h_best"] for k in range(4)] == [100, 101, 40, 41]
    p, rows = tag["match_5"]
    assert D[(0, p)]["h_best"] == D[(0, p)]["h_second"] == 0 and D[(0, p)]["best"] == min(rows)
    for p, k, row in tag["on_level"]:
        assert c["dist"][p, 1] == _pow(prm, k) * D[(0, p)]["dist"] and D[(0, p)]["level"] == k and D[(0, p)]["candidates"] == [row]
    # without status and select the points that were left out come in and win the keypoints laid on them
    e2 = sc.restate(c, True, True, False, False)
    assert [e2["verdict"].get((0, p)) for p in tag["not_searchable"]] == [None, sr.WON, sr.WON, None]


def test_census_of_the_windows():
    c = sc.windows()
    e, tag = sc.restate(c), c["tag"]
    V, D = e["verdict"], e["detail"]
    for n, (p, rows) in tag["crowd"].items():
        det = D[(0, p)]
        assert sorted(det["candidates"]) == sorted(rows) and len(rows) == n and V[(0, p)] == sr.WON and det["h_best"] == 30
        assert det["level"] == 7 and 44.0 < det["radius"] < 45.0
    for name in ("one_cell", "two_cells", "two_cells_y"):
        p, rows = tag[name]
        assert sorted(D[(0, p)]["candidates"]) == sorted(rows) and e["row_point"][rows[0]] == p
    p, rows = tag["identical"]
    assert sorted(D[(0, p)]["candidates"]) == sorted(rows) and D[(0, p)]["h_best"] == D[(0, p)]["h_second"] == 17
    assert e["row_point"][min(rows)] == p and all(e["row_inlier"][r] == 0 for r in rows if r != min(rows))
    for p, row in tag["over"]:
        x, y = (float(c["kps"][0, row, j]) for j in (0, 1))
        assert not (0 <= x < 640 and 0 <= y < 480) and row in D[(0, p)]["candidates"] and e["row_point"][row] == p
    assert float(c["kps"][0, tag["over"][0][1], 0]) == -3.0 and D[(0, tag["over"][0][0])]["u"] < 1.01
    p, rows = tag["octaves"]
    assert D[(0, p)]["candidates"] == [rows[0]] and V[(0, p)] == sr.WON  # octave -1 at level 0, alone: second octave -1 too
    assert all(V[(2, q)] in (sr.NO_CANDIDATE, sr.BEHIND) for q in range(c["n_points"]))  # the frame with the negative count
    assert not any(f == 1 for f, _ in V)


@pytest.mark.parametrize("rule", sr.RULES)
def test_the_cases_tell_a_near_rule_apart(rule):
    changed = []
    for c in CASES.values():
        a, b = sc.as_arrays(sc.restate(c), c["n_frames"]), sc.as_arrays(sc.restate(c, rule=rule), c["n_frames"])
        if any(a[k].tobytes() != b[k].tobytes() for k in ("row_point", "row_inlier", "row_dist")):
            changed.append(c["name"])
    print(rule, "changes the node outputs of", changed)
    assert changed, rule
