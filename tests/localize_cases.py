"""Inputs for gh_pnp_gather_pairs_dev: a named census on 6 frames x 8 rows (frames 0 .. 2 hold the map, frames 3 .. 5 are new;
each case a few rows of a handful of pairs), a hub (one query node voted on by 256 pairs) and a random case of 40 frames x 128
rows.  tests/test_localize_cpu.py shows what they reach; tests/test_localize_gpu.py holds the device to
tests/localize_restate.py on them, byte for byte."""
import functools

import numpy as np

import localize_restate as lr

N_FRAMES, CAP, N_POINTS = 6, 8, 6
INTRINSICS = (517.3, 516.5, 318.6, 255.3)
INT32_MAX = 2**31 - 1
FILL = 0xA5  # every byte of every output buffer before a call

# The census map.  Frames 0 and 1 see point r at row r, frame 2 sees the points in reverse; rows 6 and 7 hold the codes
# gh_link_tracks_dev writes where there is no point.  The new frames hold VALID ids (1, 2, 3): the contract reads a frame's
# entries only where the frame is the train frame of a pair, so they show only in the case made for that.
NODE_POINT = np.array([[0, 1, 2, 3, 4, 5, -1, -2],
                       [0, 1, 2, 3, 4, 5, -1, -3],
                       [5, 4, 3, 2, 1, 0, -2, -1],
                       [1] * 8, [2] * 8, [3] * 8], np.int32)


def make_kps(n_frames, cap, seed):
    """n_frames x cap x 7 float32 view of KeyPoint records: x, y random pixels, the other fields zero."""
    rng = np.random.default_rng(seed)
    kps = np.zeros((n_frames, cap, 7), np.float32)
    kps[..., 0] = rng.uniform(0.0, 640.0, (n_frames, cap)).astype(np.float32)
    kps[..., 1] = rng.uniform(0.0, 480.0, (n_frames, cap)).astype(np.float32)
    return kps


def make_points(n_points, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(-5.0, 5.0, (n_points, 3)))


def _case(name, pairs, counts=None, node_point=None, n_points=N_POINTS, status=None):
    """pairs: [(q, t, {row: idx1}, [rows whose keep byte is 0])]; rows not listed hold idx1 = -1, keep = 1."""
    P = len(pairs)
    idx1 = np.full((P, CAP), -1, np.int32)
    keep = np.ones((P, CAP), np.uint8)
    for p, (_, _, rows, off) in enumerate(pairs):
        for i, j in rows.items():
            idx1[p, i] = j
        for i in off:
            keep[p, i] = 0
    return dict(name=name, n_frames=N_FRAMES, cap=CAP, kps=make_kps(N_FRAMES, CAP, 21),
                counts=np.array([CAP] * N_FRAMES if counts is None else counts, np.int32),
                pair_q=np.array([p[0] for p in pairs], np.int32), pair_t=np.array([p[1] for p in pairs], np.int32),
                idx1=idx1, keep=keep, node_point=(NODE_POINT if node_point is None else np.array(node_point, np.int32)).reshape(-1).copy(),
                point_xyz=make_points(n_points, 22), status=np.array([0] * n_points if status is None else status, np.int32))


def census():
    past = NODE_POINT.copy()
    past[0] = [N_POINTS - 1, N_POINTS, N_POINTS + 1, INT32_MAX, -INT32_MAX - 1, -4, -1, -2]
    return [
        # row 0 sees point 0; row 1 hits a train row without a point, row 2 a train row that does not match: NO_POINT
        _case("correspondence_and_no_point", [(3, 0, {0: 0, 1: 6, 2: -1}, [])]),
        # frame 0 says point 0, frame 2 says point 5: dropped, not voted on -- also with two votes against one
        _case("two_pairs_disagree", [(3, 0, {0: 0, 4: 4}, []), (3, 2, {0: 0}, []), (4, 0, {1: 2}, []), (4, 1, {1: 2}, []), (4, 2, {1: 2}, [])]),
        # frames 0, 1 and 2 (row 3 there holds point 2) agree on point 2
        _case("two_pairs_agree", [(3, 0, {0: 2}, []), (3, 1, {0: 2}, []), (3, 2, {0: 3}, [])]),
        _case("same_pair_twice", [(3, 0, {1: 1}, []), (3, 0, {1: 1}, [])]),
        # rows 0 and 1 both hit point 4, rows 3, 4, 5 all hit point 3; row 2 alone sees point 2
        _case("many_to_one_inside_one_pair", [(3, 0, {0: 4, 1: 4, 2: 2, 3: 3, 4: 3, 5: 3}, [])]),
        # every pair is one-to-one: row 0 sees point 1 in frame 0, row 1 sees point 1 in frame 2 (row 4 there)
        _case("many_to_one_through_two_map_frames", [(3, 0, {0: 1}, []), (3, 2, {1: 4}, [])]),
        # point 0 claimed by one row each of frames 3, 4 and 5: neighbours in the sorted list, different frames, all stay
        _case("same_point_from_rows_of_different_frames", [(3, 0, {0: 0}, []), (4, 0, {5: 0}, []), (5, 1, {7: 0}, [])]),
        # row 0 is AMBIGUOUS between points 0 and 5 and claims nothing: row 1, which sees point 0, is not SHARED with it
        _case("ambiguous_row_claims_nothing", [(3, 0, {0: 0, 1: 0}, [0]), (3, 0, {0: 0}, []), (3, 2, {0: 0}, [])]),
        # n_points - 1 is the last id; n_points, n_points + 1, INT32_MAX, INT32_MIN and other negatives drop the candidate
        _case("candidate_at_and_past_n_points", [(3, 0, {i: i for i in range(8)}, [])], node_point=past),
        # only points 0 and 3 are GH_TRACK_OK (with the status NULL all of them count)
        _case("status_other_than_ok", [(3, 0, {i: i for i in range(6)}, [])], status=[0, 1, 2, 0, 4, 5]),
        # idx1 of -1, counts[t], cap and INT32_MAX drop the row; counts[t] - 1 is the last valid one
        _case("idx1_out_of_range", [(3, 1, {0: -1, 1: 5, 2: CAP, 3: INT32_MAX, 4: 4}, [])], counts=[8, 5, 8, 8, 8, 8]),
        # a query row at counts[q] is ignored (and is NO_ROW), the one at counts[q] - 1 is read
        _case("query_row_at_the_count", [(3, 0, {3: 3, 2: 2}, [])], counts=[8, 8, 8, 3, 8, 8]),
        # counts -3 -> 0 and cap + 5 -> cap; frame 2 holds nothing: nothing is read from frames 0 and 2, nothing for frame 4
        _case("clamped_and_empty_counts", [(3, 1, {7: 5}, []), (3, 0, {0: 1}, []), (5, 2, {2: 0}, []), (4, 1, {0: 0}, []), (5, 1, {6: 4}, [])],
              counts=[-3, CAP + 5, 0, 8, -1, 8]),
        _case("pair_index_out_of_range", [(6, 1, {0: 0}, []), (-1, 2, {0: 0}, []), (3, 7, {1: 1}, []), (3, INT32_MAX, {1: 1}, []),
                                          (-INT32_MAX - 1, 0, {1: 1}, []), (4, 1, {1: 1}, [])]),
        _case("pair_of_a_frame_with_itself", [(3, 3, {0: 1}, []), (0, 0, {0: 1}, []), (3, 1, {5: 5}, [])]),
        # the keep byte 0 sits on the row that would make row 0 AMBIGUOUS
        _case("keep_zero", [(3, 0, {0: 0, 1: 1}, []), (3, 2, {0: 0, 1: 4}, [0])]),
        # frame 3 is the query of pair 0 and the train of pair 1: frame 4 reads node_point of frame 3 as it was GIVEN (point 1),
        # not what this call finds for frame 3 (point 0)
        _case("query_and_train_at_once", [(3, 0, {0: 0}, []), (4, 3, {0: 0}, []), (0, 3, {2: 2}, [])]),
        _case("no_candidates_at_all", [(3, 0, {}, [])]),
    ]


def hub(dissenter=None):
    """257 frames x 2 rows: row 0 of frame 256 matched to row 0 of each of the 256 map frames, which all hold point 7;
    dissenter: the pair whose map frame holds another point there (a lower id for an even pair, a higher for an odd one)."""
    n_frames, cap, n_points = 257, 2, 10
    pt = np.arange(n_frames - 1, dtype=np.int32)
    idx1 = np.full((n_frames - 1, cap), -1, np.int32)
    idx1[:, 0] = 0
    node_point = np.full((n_frames, cap), -1, np.int32)
    node_point[:-1, 0] = 7
    if dissenter is not None:
        node_point[dissenter, 0] = 3 if dissenter % 2 == 0 else 9
    return dict(name="hub" if dissenter is None else "hub_dissenter_%d" % dissenter, n_frames=n_frames, cap=cap,
                kps=make_kps(n_frames, cap, 23), counts=np.full(n_frames, cap, np.int32), pair_q=np.full(n_frames - 1, n_frames - 1, np.int32),
                pair_t=pt, idx1=idx1, keep=np.ones((n_frames - 1, cap), np.uint8), node_point=node_point.reshape(-1),
                point_xyz=make_points(n_points, 24), status=np.zeros(n_points, np.int32))


HUB_DISSENTERS = (0, 127, 255)


def random_map(n_frames=40, n_map=30, cap=128, n_points=300, per_new=12, seed=9, seen=0.2, wrong=0.03, stray=0.01):
    """Ground-truth points, each seen by a frame with probability `seen` at a random free row; frames 0 .. n_map - 1 hold the map,
    every later frame is matched against `per_new` random map frames; the share `wrong` of the matched rows redirected to a random
    row (AMBIGUOUS where another pair says otherwise); the share `stray` of the rows without a match sent to a random row, as a
    matcher without a cross check does (SHARED where that point has its own row in the frame); a tenth of the points are not GH_TRACK_OK, a tenth of the map's observations carry a code instead of the id, and node_point is dirty wherever
    the contract does not read it or must reject what it reads."""
    rng = np.random.default_rng(seed)
    row_of = -np.ones((n_frames, n_points), np.int64)
    for f in range(n_frames):
        pts = np.flatnonzero(rng.random(n_points) < seen)
        row_of[f, pts] = rng.permutation(cap)[:len(pts)]
    dirt = np.array([-1, -2, -3, -4, -77, n_points, n_points + 5, INT32_MAX, -INT32_MAX - 1], np.int64)
    node_point = dirt[rng.integers(0, len(dirt), (n_frames, cap))]
    for f in range(n_map):
        pts = np.flatnonzero(row_of[f] >= 0)
        pts = pts[rng.random(len(pts)) >= 0.1]
        node_point[f, row_of[f, pts]] = pts
    node_point[n_map:] = rng.integers(0, n_points, (n_frames - n_map, cap))  # valid ids, never to be read
    pairs = [(q, int(t)) for q in range(n_map, n_frames) for t in rng.permutation(n_map)[:per_new]]
    idx1 = np.full((len(pairs), cap), -1, np.int32)
    for k, (q, t) in enumerate(pairs):
        both = np.flatnonzero((row_of[q] >= 0) & (row_of[t] >= 0))
        idx1[k, row_of[q, both]] = row_of[t, both]
    matched = np.argwhere(idx1 >= 0)
    for k, i in matched[rng.random(len(matched)) < wrong]:
        idx1[k, i] = rng.integers(0, cap)
    unmatched = np.argwhere(idx1 < 0)
    for k, i in unmatched[rng.random(len(unmatched)) < stray]:
        idx1[k, i] = rng.integers(0, cap)
    keep = (rng.random(idx1.shape) >= 0.02).astype(np.uint8)
    counts = np.full(n_frames, cap, np.int32)
    counts[[3, n_map + 2]] = cap - 9
    status = np.where(rng.random(n_points) < 0.1, rng.integers(1, 6, n_points), 0).astype(np.int32)
    return dict(name="random_map", n_frames=n_frames, cap=cap, kps=make_kps(n_frames, cap, seed + 1), counts=counts,
                pair_q=np.array([p[0] for p in pairs], np.int32), pair_t=np.array([p[1] for p in pairs], np.int32), idx1=idx1, keep=keep,
                node_point=node_point.astype(np.int32).reshape(-1), point_xyz=make_points(n_points, seed + 2), status=status)


def reorder(c, order, seed=0):
    """The same case with its pair list in another order: forward, reversed or shuffled."""
    P = len(c["pair_q"])
    perm = {"forward": np.arange(P), "reversed": np.arange(P)[::-1], "shuffled": np.random.default_rng(seed).permutation(P)}[order]
    return dict(c, pair_q=c["pair_q"][perm].copy(), pair_t=c["pair_t"][perm].copy(), idx1=c["idx1"][perm].copy(), keep=c["keep"][perm].copy())


def restate(c, use_keep=True, use_status=True, intrinsics=INTRINSICS):
    """tests/localize_restate.py on a case -> its dict of lists."""
    return lr.gather(c["kps"][..., :2], c["counts"].tolist(), c["n_frames"], c["cap"], c["pair_q"].tolist(), c["pair_t"].tolist(),
                     c["idx1"].reshape(-1).tolist(), c["keep"].reshape(-1).tolist() if use_keep else None, c["node_point"].tolist(),
                     c["point_xyz"].tolist(), c["status"].tolist() if use_status else None, intrinsics)


@functools.lru_cache(maxsize=None)
def random_case():
    """The random case and its restatement (with keep and status, and without both), computed once per session and left
    unchanged."""
    c = random_map()
    return c, restate(c, True, True), restate(c, False, False)


@functools.lru_cache(maxsize=None)
def hub_cases():
    out = []
    for d in (None,) + HUB_DISSENTERS:
        c = hub(d)
        out.append((c, restate(c)))
    return out


def as_arrays(e, n_frames, cap):
    """The restatement's lists as the arrays the device writes."""
    N = n_frames * cap
    return dict(row_point=np.array(e["row_point"], np.int32).reshape(N), offsets=np.array(e["offsets"], np.int32).reshape(n_frames + 1),
                xyz=np.array(e["xyz"], np.float64).reshape(N, 3), xy=np.array(e["xy"], np.float64).reshape(N, 2),
                corr_node=np.array(e["corr_node"], np.int32).reshape(N), totals=np.array(e["totals"], np.int32))


SCENE_MAP, SCENE_NEW, SCENE_CAP, SCENE_F, SCENE_C = 6, 3, 256, 500.0, (320.0, 240.0)
SCENE_RANSAC_THRESHOLD, SCENE_INLIER_THRESHOLD, SCENE_SEED = 0.006, 0.006, 11


@functools.lru_cache(maxsize=None)
def scene():
    """6 map frames and 3 new frames of a synthetic graph of 150 points with known poses, exact pixels (rounded to float32) and
    exact matches: `map_pairs` (all 15 pairs of map frames) build the map, `new_pairs` (every new frame against every map frame)
    localise.  A tenth of the matched rows of every new frame are PLANTED wrong: in every pair the row goes to the train row of
    one other point, one that neither the new frame itself sees nor another planted row of it was sent to (so the row is a
    correspondence, not SHARED) and whose projection in the new frame lies farthest from the row's pixel.  -> dict of host arrays; planted: new frame x cap bool; planted_error: the
    smallest distance, in normalised units, between a planted row and the projection of the point it was sent to."""
    from gslam_amd import ba_synth
    n_cams, n_pts, cap = SCENE_MAP + SCENE_NEW, 150, SCENE_CAP
    g = ba_synth.make_graph(n_cams, n_pts, 6, seed=4, noise=0.0, outlier_frac=0.0, perturb=False)
    per_cam = [np.flatnonzero(g["obs_cam"] == cam) for cam in range(n_cams)]
    kps = np.zeros((n_cams, cap, 7), np.float32)
    row_of = -np.ones((n_cams, n_pts), np.int64)
    for cam, obs in enumerate(per_cam):
        assert len(obs) <= cap
        kps[cam, :len(obs), 0] = (SCENE_F * g["obs_xy"][obs, 0] + SCENE_C[0]).astype(np.float32)
        kps[cam, :len(obs), 1] = (SCENE_F * g["obs_xy"][obs, 1] + SCENE_C[1]).astype(np.float32)
        row_of[cam, g["obs_point"][obs]] = np.arange(len(obs))
    counts = np.array([len(o) for o in per_cam], np.int32)

    def exact(pairs, send=None):
        idx1 = np.full((len(pairs), cap), -1, np.int32)
        for k, (q, t) in enumerate(pairs):
            for p in np.flatnonzero(row_of[q] >= 0):
                seen_as = p if send is None else send.get((q, int(p)), p)
                if row_of[t, seen_as] >= 0:
                    idx1[k, row_of[q, p]] = row_of[t, seen_as]
        return idx1

    map_pairs = [(q, t) for q in range(SCENE_MAP) for t in range(q + 1, SCENE_MAP)]
    new_pairs = [(q, t) for q in range(SCENE_MAP, n_cams) for t in range(SCENE_MAP)]
    rng = np.random.default_rng(5)
    send, planted, planted_error = {}, np.zeros((n_cams, cap), bool), np.inf
    Rq = ba_synth.quat_to_R(g["cam_pose_gt"][:, :4])
    for q in range(SCENE_MAP, n_cams):
        Xc = (g["point_xyz_gt"] - g["cam_pose_gt"][q, 4:]) @ Rq[q]
        proj = Xc[:, :2] / Xc[:, 2:3]
        mapped = (row_of[:SCENE_MAP] >= 0).sum(0) >= 2
        unseen = np.flatnonzero((row_of[q] < 0) & mapped)
        for p in np.flatnonzero((row_of[q] >= 0) & (rng.random(n_pts) < 0.1)):
            far = np.linalg.norm(proj[unseen] - proj[p], axis=1)
            send[(q, int(p))] = int(unseen[far.argmax()])
            planted[q, row_of[q, p]] = True
            planted_error = min(planted_error, far.max())
            unseen = np.delete(unseen, far.argmax())  # (two rows sent to one point would be SHARED)
    return dict(n_frames=n_cams, cap=cap, kps=kps, counts=counts, poses=np.ascontiguousarray(g["cam_pose_gt"]),
                map_q=np.array([p[0] for p in map_pairs], np.int32), map_t=np.array([p[1] for p in map_pairs], np.int32),
                map_idx1=exact(map_pairs), new_q=np.array([p[0] for p in new_pairs], np.int32),
                new_t=np.array([p[1] for p in new_pairs], np.int32), new_idx1=exact(new_pairs, send), planted=planted,
                planted_error=float(planted_error), intrinsics=(SCENE_F, SCENE_F) + SCENE_C)
