"""Inputs for gh_extend_tracks_dev: a hand-built census on 6 frames x 8 rows, a hub (one point adopted from 256 frames), a chain
(one new track through 64 frames), a random map that grows by ten frames, a random soup at the block boundaries N = 512 and
N = 513, and the synthetic scene of localize_cases with pairs among its new frames.  tests/test_track_extend_cpu.py shows what
they reach; tests/test_track_extend_gpu.py holds the device to tests/track_extend_restate.py on them, byte for byte."""
import functools

import numpy as np

import localize_cases as loc
import localize_restate as locr
import track_extend_restate as er
import track_link_cases as lc
import track_link_restate as lr

INTRINSICS = lc.INTRINSICS
INT32_MAX = 2**31 - 1
OUTPUTS = ("node_point", "obs_cam", "obs_point", "obs_xy", "obs_node", "point_len", "point_new", "point_grew", "totals")


def _pairs(pairs, cap):
    """pairs: [(q, t, {row: idx1}, [rows whose inlier byte is 0])]; rows not listed hold idx1 = -1, inlier = 1."""
    idx1 = np.full((len(pairs), cap), -1, np.int32)
    inlier = np.ones((len(pairs), cap), np.uint8)
    for p, (_, _, rows, off) in enumerate(pairs):
        for i, j in rows.items():
            idx1[p, i] = j
        for i in off:
            inlier[p, i] = 0
    return dict(pair_q=np.array([p[0] for p in pairs], np.int32), pair_t=np.array([p[1] for p in pairs], np.int32), idx1=idx1, inlier=inlier)


def census():
    """Frames 0 .. 2 hold the map of n_points = 5 points, frames 3 .. 5 are new; frame 5 has 6 rows.  What every row is for:
      map       point 0 at (0,0) (1,0) (2,0); point 1 at (0,1) (1,1); point 2 at (0,2) (1,2) and at the new frame's (3,7); point 3 at
                (1,3) (2,1); point 4 nowhere.  (0,4) holds a link code, (0,5) n_points, (0,6) INT32_MAX: no point, FREE.
      ADOPTED   (3,0) (4,0) (5,0) adopt point 0 -- three frames, one point; (4,6) adopts point 2.  (0,0) is MAPPED and carries a
                claim of point 3 as well: MAPPED is checked first.
      REJECTED  (3,1) claims point 2, which (3,7) holds; (4,1) (4,2) both claim point 1; (4,3) (4,4) (4,5) all claim point 3;
                (5,1) (5,2) both claim point 4, which therefore ends with no observation at all.
      FREE      (3,2) claims point 1 with row_inlier 0; (3,3) claims -1, (3,4) claims n_points, (3,5) claims -4; the rows
                (5,6) (5,7) do not exist and claim point 0 with row_inlier 1: NO_ROW, and (5,0) is not rejected for them.
      edges     TRACK (3,2)-(4,7)-(5,3); (3,3)-(1,4) is a track for min_views = 2 and SHORT of two nodes for 3; the edge (3,3)-(0,0)
                FREE-MAPPED, (5,4)-(3,0) FREE-ADOPTED and (5,4)-(4,1) FREE-REJECTED are ignored, so (5,4) stays alone;
                CONFLICT (3,4) (3,5) -> (2,5); (0,3)-(1,5) only without the inlier bytes."""
    F, cap, n_points = 6, 8, 5
    node_point = np.full((F, cap), -1, np.int32)
    node_point[0, :7] = [0, 1, 2, -1, -2, n_points, INT32_MAX]
    node_point[1, :4] = [0, 1, 2, 3]
    node_point[2, :2] = [0, 3]
    node_point[3, 7] = 2
    node_point[4, 7] = -3
    row_point = np.full((F, cap), -1, np.int32)
    row_inlier = np.zeros((F, cap), np.uint8)
    claims = {(0, 0): (3, 1), (3, 0): (0, 1), (3, 1): (2, 1), (3, 2): (1, 0), (3, 3): (-1, 1), (3, 4): (n_points, 1), (3, 5): (-4, 1),
              (4, 0): (0, 1), (4, 1): (1, 1), (4, 2): (1, 1), (4, 3): (3, 1), (4, 4): (3, 1), (4, 5): (3, 1), (4, 6): (2, 1),
              (5, 0): (0, 1), (5, 1): (4, 1), (5, 2): (4, 1), (5, 6): (0, 1), (5, 7): (0, 1)}
    for (f, i), (c, b) in claims.items():
        row_point[f, i], row_inlier[f, i] = c, b
    pairs = [(4, 3, {7: 2}, []), (5, 4, {3: 7, 4: 1}, []), (3, 0, {3: 0}, []), (3, 1, {3: 4}, []), (5, 3, {4: 0}, []),
             (3, 2, {4: 5, 5: 5}, []), (0, 1, {3: 5}, [3])]
    return dict(name="census", n_frames=F, cap=cap, kps=lc.make_kps(F, cap, 31), counts=np.array([8, 8, 8, 8, 8, 6], np.int32),
                node_point=node_point.reshape(-1), n_points=n_points, row_point=row_point.reshape(-1), row_inlier=row_inlier.reshape(-1),
                min_views=3, **_pairs(pairs, cap))


def hub(mapped_in_frame_128=False):
    """257 frames x 4 rows, n_points = 3.  Frame 0 holds point 1 at row 0; row 0 of every frame 1 .. 256 claims point 1: one
    point adopted from 256 frames.  Row 1 of every frame 1 .. 256 is matched to row 1 of frame 0: one new track of 257 views,
    contended by 256 unions.  The variant: frame 128 holds point 1 at row 2 already, so its claimant is REJECTED."""
    F, cap, n_points = 257, 4, 3
    node_point = np.full((F, cap), -1, np.int32)
    node_point[0, 0] = 1
    if mapped_in_frame_128:
        node_point[128, 2] = 1
    row_point = np.full((F, cap), -1, np.int32)
    row_inlier = np.zeros((F, cap), np.uint8)
    row_point[1:, 0], row_inlier[1:, 0] = 1, 1
    idx1 = np.full((F - 1, cap), -1, np.int32)
    idx1[:, 0], idx1[:, 1] = 0, 1
    return dict(name="hub_mapped_128" if mapped_in_frame_128 else "hub", n_frames=F, cap=cap, kps=lc.make_kps(F, cap, 32),
                counts=np.full(F, cap, np.int32), node_point=node_point.reshape(-1), n_points=n_points, row_point=row_point.reshape(-1),
                row_inlier=row_inlier.reshape(-1), min_views=2, pair_q=np.arange(1, F, dtype=np.int32), pair_t=np.zeros(F - 1, np.int32),
                idx1=idx1, inlier=np.ones((F - 1, cap), np.uint8))


def reorder(c, order, seed=0):
    """The same case with its pair list in another order: forward, reversed or shuffled."""
    P = len(c["pair_q"])
    perm = {"forward": np.arange(P), "reversed": np.arange(P)[::-1], "shuffled": np.random.default_rng(seed).permutation(P)}[order]
    return dict(c, pair_q=c["pair_q"][perm].copy(), pair_t=c["pair_t"][perm].copy(), idx1=c["idx1"][perm].copy(), inlier=c["inlier"][perm].copy())


def chain():
    """66 frames x 4 rows, n_points = 2.  Frames 0 and 1 hold point 0 at row 0; row 0 of every later frame adopts it.  Row 1 of
    frame f is matched to row 1 of frame f + 1 for f = 2 .. 64: ONE new track through the 64 new frames.  Row 2 is matched the
    same way from frame 0 on: a second new track, 66 views, that takes in FREE rows of the map frames.  The matches of row 0
    have a MAPPED or ADOPTED node on both ends and are ignored."""
    F, cap, n_points = 66, 4, 2
    node_point = np.full((F, cap), -1, np.int32)
    node_point[:2, 0] = 0
    row_point = np.full((F, cap), -1, np.int32)
    row_inlier = np.zeros((F, cap), np.uint8)
    row_point[2:, 0], row_inlier[2:, 0] = 0, 1
    pq = np.arange(F - 1, dtype=np.int32)
    idx1 = np.full((F - 1, cap), -1, np.int32)
    idx1[:, 0] = 0      # MAPPED / ADOPTED rows on both ends: ignored
    idx1[2:, 1] = 1
    idx1[:, 2] = 2
    return dict(name="chain", n_frames=F, cap=cap, kps=lc.make_kps(F, cap, 33), counts=np.full(F, cap, np.int32),
                node_point=node_point.reshape(-1), n_points=n_points, row_point=row_point.reshape(-1), row_inlier=row_inlier.reshape(-1),
                min_views=2, pair_q=pq, pair_t=pq + 1, idx1=idx1, inlier=np.ones((F - 1, cap), np.uint8))


def random_growth(n_frames=40, n_map=30, cap=64, n_truth=280, neighbours=6, seed=5, wrong_claim=0.02, duplicate_claim=0.01, outlier=0.1):
    """track_link_cases.random_windows (3 % wrong matches, 2 % of the inlier bytes 0) split in time: the pairs inside the first
    n_map frames build the map with the restated link; the pairs of a later frame with a map frame give the claims through the
    restated gather; row_inlier is 1 at nine tenths of the correspondences; then wrong_claim of the rows of the new frames claim
    a random point, and duplicate_claim of them repeat the claim of a claiming row of their frame.  The call gets every pair that
    touches a new frame."""
    c = lc.random_windows(n_frames=n_frames, cap=cap, n_points=n_truth, seed=seed, neighbours=neighbours)
    rng = np.random.default_rng(seed + 100)
    N = n_frames * cap
    q, t = c["pair_q"], c["pair_t"]
    old = (q < n_map) & (t < n_map)
    m = lr.link(c["kps"][..., :2], c["counts"].tolist(), n_frames, cap, q[old].tolist(), t[old].tolist(), c["idx1"][old].reshape(-1).tolist(),
                c["inlier"][old].reshape(-1).tolist(), INTRINSICS, 2)
    n_points = m["totals"][1]
    node_point = np.array(m["node_point"], np.int32)
    cross = (q >= n_map) & (t < n_map)
    g = locr.gather(c["kps"][..., :2], c["counts"].tolist(), n_frames, cap, q[cross].tolist(), t[cross].tolist(),
                    c["idx1"][cross].reshape(-1).tolist(), c["inlier"][cross].reshape(-1).tolist(), node_point.tolist(),
                    [(0.0, 0.0, 0.0)] * n_points, None, INTRINSICS)
    row_point = np.array(g["row_point"], np.int32)
    row_inlier = ((row_point >= 0) & (rng.random(N) >= outlier)).astype(np.uint8)
    new_nodes = np.arange(n_map * cap, N)
    for n in new_nodes[rng.random(len(new_nodes)) < wrong_claim]:
        row_point[n], row_inlier[n] = rng.integers(0, n_points), 1
    for n in new_nodes[rng.random(len(new_nodes)) < duplicate_claim]:
        claiming = np.flatnonzero(row_point[(n // cap) * cap:(n // cap + 1) * cap] >= 0)
        if len(claiming):
            row_point[n], row_inlier[n] = row_point[(n // cap) * cap + int(rng.choice(claiming))], 1
    new = ~old
    return dict(name="random_growth", n_frames=n_frames, cap=cap, kps=c["kps"], counts=c["counts"], node_point=node_point, n_points=n_points,
                row_point=row_point, row_inlier=row_inlier, min_views=2, pair_q=q[new].copy(), pair_t=t[new].copy(),
                idx1=c["idx1"][new].copy(), inlier=c["inlier"][new].copy())


def soup(n_frames, cap, counts, n_points=9, seed=7):
    """Random everything, valid or not: node_point and row_point drawn from the ids and from values the contract must turn
    down, idx1 from -1 .. cap, every frame paired with the next two.  The LAST existing node of the last frame is MAPPED and the
    first node adopts (the last id, which nothing else draws), so the first and the last lane of the node range both carry an observation."""
    rng = np.random.default_rng(seed)
    N = n_frames * cap
    values = np.array(list(range(n_points - 1)) * 2 + [-1, -1, -1, -1, -2, -3, -4, n_points, INT32_MAX, -INT32_MAX - 1], np.int64)
    node_point = np.where(rng.random(N) < 0.35, values[rng.integers(0, len(values), N)], -1)
    node_point[(n_frames // 2) * cap:] = np.where(rng.random(N - (n_frames // 2) * cap) < 0.9, -1, node_point[(n_frames // 2) * cap:])
    row_point = values[rng.integers(0, len(values), N)]
    row_inlier = (rng.random(N) < 0.4).astype(np.uint8) * rng.integers(1, 256, N).astype(np.uint8)
    counts = np.array(counts, np.int32)
    node_point[(n_frames - 1) * cap + int(counts[-1]) - 1] = 0
    node_point[0], row_point[0], row_inlier[0] = -1, n_points - 1, 1
    pairs = [(f, f + d) for f in range(n_frames) for d in (1, 2) if f + d < n_frames]
    idx1 = np.where(rng.random((len(pairs), cap)) < 0.5, rng.integers(-1, cap + 1, (len(pairs), cap)), -1).astype(np.int32)
    inlier = (rng.random(idx1.shape) >= 0.1).astype(np.uint8)
    return dict(name="soup_%dx%d" % (n_frames, cap), n_frames=n_frames, cap=cap, kps=lc.make_kps(n_frames, cap, seed + 1), counts=counts,
                node_point=node_point.astype(np.int32), n_points=n_points, row_point=row_point.astype(np.int32), row_inlier=row_inlier,
                min_views=2, pair_q=np.array([p[0] for p in pairs], np.int32), pair_t=np.array([p[1] for p in pairs], np.int32), idx1=idx1,
                inlier=inlier)


def boundaries():
    """N = 512 (two workgroups exactly; the flags cover N + 1 = 513 entries) and N = 513 (one node into the third)."""
    return [soup(8, 64, [64] * 8), soup(3, 171, [171, 171, 170])]


def restate(c, use_inlier=True, use_map=True, use_claims=True, min_views=None, intrinsics=INTRINSICS):
    """tests/track_extend_restate.py on a case -> its dict of lists."""
    return er.extend(c["kps"][..., :2], c["counts"].tolist(), c["n_frames"], c["cap"], c["pair_q"].tolist(), c["pair_t"].tolist(),
                     c["idx1"].reshape(-1).tolist(), c["inlier"].reshape(-1).tolist() if use_inlier else None,
                     c["node_point"].tolist() if use_map and c["node_point"] is not None else None, c["n_points"],
                     c["row_point"].tolist() if use_claims and c["row_point"] is not None else None,
                     c["row_inlier"].tolist() if use_claims and c["row_inlier"] is not None else None, intrinsics,
                     c["min_views"] if min_views is None else min_views)


@functools.lru_cache(maxsize=None)
def random_case():
    """The random case and its restatement (with the inlier bytes and without), computed once per session and left unchanged."""
    c = random_growth()
    return c, restate(c, True), restate(c, False)


def as_arrays(e, N, PC):
    """The restatement's lists as the arrays the device writes."""
    return dict(node_point=np.array(e["node_point"], np.int32).reshape(N), obs_cam=np.array(e["obs_cam"], np.int32).reshape(N),
                obs_point=np.array(e["obs_point"], np.int32).reshape(N), obs_xy=np.array(e["obs_xy"], np.float64).reshape(N, 2),
                obs_node=np.array(e["obs_node"], np.int32).reshape(N), point_len=np.array(e["point_len"], np.int32).reshape(PC),
                point_new=np.array(e["point_new"], np.uint8).reshape(PC), point_grew=np.array(e["point_grew"], np.uint8).reshape(PC),
                totals=np.array(e["totals"], np.int32))


@functools.lru_cache(maxsize=None)
def scene(late_points=False):
    """localize_cases.scene() and what the extension needs on top of it, from the same graph: `ext_q`, `ext_t`, `ext_idx1` are the
    new-versus-map pairs of the scene (planted rows included) followed by the exact pairs among the three new frames, in which
    the planted rows take no part on either side (a planted row is a keypoint whose descriptor is wrong: the scene sends it to
    another point in every pair, and two of them must not find each other); `true_point` (frame x cap, -1 where the row is
    empty) is the graph's point behind every keypoint row.
    Every point of the scene is seen by at least three of the six map frames, so the map holds all of them and nothing new can
    appear.  late_points: every fourth point that no planted row was sent to is taken out of the map pairs -- the map frames
    see it, but the matcher has not linked it yet -- so the map does not hold it (`late`: point -> bool) and the new frames
    bring it in: its rows in the new frames, and the rows of the map frames they are matched to, become a new track."""
    from gslam_amd import ba_synth
    s = loc.scene()
    n_cams, cap, n_pts = s["n_frames"], s["cap"], 150
    g = ba_synth.make_graph(n_cams, n_pts, 6, seed=4, noise=0.0, outlier_frac=0.0, perturb=False)
    true_point = -np.ones((n_cams, cap), np.int64)
    row_of = -np.ones((n_cams, n_pts), np.int64)
    for cam in range(n_cams):
        pts = g["obs_point"][np.flatnonzero(g["obs_cam"] == cam)]
        true_point[cam, :len(pts)] = pts
        row_of[cam, pts] = np.arange(len(pts))
    assert ((row_of[:loc.SCENE_MAP] >= 0).sum(0) >= 3).all()
    planted = s["planted"]
    new_pairs = [(q, t) for q in range(loc.SCENE_MAP, n_cams) for t in range(q + 1, n_cams)]
    idx1 = np.full((len(new_pairs), cap), -1, np.int32)
    for k, (q, t) in enumerate(new_pairs):
        both = np.flatnonzero((row_of[q] >= 0) & (row_of[t] >= 0))
        both = both[~planted[q, row_of[q, both]] & ~planted[t, row_of[t, both]]]
        idx1[k, row_of[q, both]] = row_of[t, both]
    late = np.zeros(n_pts, bool)
    map_idx1 = s["map_idx1"]
    if late_points:
        sent_to = set()
        for k, (q, t) in enumerate(zip(s["new_q"].tolist(), s["new_t"].tolist())):
            rows = np.flatnonzero(planted[q] & (s["new_idx1"][k] >= 0))
            sent_to |= set(true_point[t, s["new_idx1"][k, rows]].tolist())
        late[[p for p in range(0, n_pts, 4) if p not in sent_to]] = True
        map_idx1 = map_idx1.copy()
        for k, q in enumerate(s["map_q"].tolist()):
            rows = np.flatnonzero(true_point[q] >= 0)
            map_idx1[k, rows[late[true_point[q, rows]]]] = -1
    return dict(s, map_idx1=map_idx1, ext_q=np.concatenate([s["new_q"], np.array([p[0] for p in new_pairs], np.int32)]),
                ext_t=np.concatenate([s["new_t"], np.array([p[1] for p in new_pairs], np.int32)]),
                ext_idx1=np.concatenate([s["new_idx1"], idx1]), true_point=true_point, late=late,
                point_xyz_gt=np.ascontiguousarray(g["point_xyz_gt"]))
