"""Inputs for gh_link_tracks_dev: a named census on 6 frames x 8 rows (each case a few rows of a handful of pairs), and the
generators of the larger cases (long chain, hub, random windows).  tests/test_track_link_cpu.py shows what they reach;
tests/test_track_link_gpu.py holds the device to tests/track_link_restate.py on them, byte for byte."""
import functools

import numpy as np

import track_link_restate as lr

N_FRAMES, CAP = 6, 8
INTRINSICS = (517.3, 516.5, 318.6, 255.3)
INT32_MAX = 2**31 - 1
FILL_BYTE, FILL_XY, FILL_INT = 0xAB, 7.0, -5  # what the output buffers hold before a call


def make_kps(n_frames, cap, seed):
    """n_frames x cap x 7 float32 view of KeyPoint records: x, y random pixels, the other fields zero."""
    rng = np.random.default_rng(seed)
    kps = np.zeros((n_frames, cap, 7), np.float32)
    kps[..., 0] = rng.uniform(0.0, 640.0, (n_frames, cap)).astype(np.float32)
    kps[..., 1] = rng.uniform(0.0, 480.0, (n_frames, cap)).astype(np.float32)
    return kps


def _case(name, pairs, counts=None, min_views=2):
    """pairs: [(q, t, {row: idx1}, [rows whose inlier byte is 0])]; rows not listed hold idx1 = -1, inlier = 1."""
    P = len(pairs)
    idx1 = np.full((P, CAP), -1, np.int32)
    inlier = np.ones((P, CAP), np.uint8)
    for p, (_, _, rows, off) in enumerate(pairs):
        for i, j in rows.items():
            idx1[p, i] = j
        for i in off:
            inlier[p, i] = 0
    return dict(name=name, n_frames=N_FRAMES, cap=CAP, kps=make_kps(N_FRAMES, CAP, 11),
                counts=np.array([CAP] * N_FRAMES if counts is None else counts, np.int32),
                pair_q=np.array([p[0] for p in pairs], np.int32), pair_t=np.array([p[1] for p in pairs], np.int32),
                idx1=idx1, inlier=inlier, min_views=min_views)


def census():
    chain = [(f, f + 1, {0: 0}, []) for f in range(5)]
    return [
        # a 6-view track on row 0, a 3-view track (0,1)-(1,2)-(2,1), a 2-view track (3,5)-(4,6)
        _case("clean_2_3_6_views", [(0, 1, {0: 0, 1: 2}, []), (1, 2, {0: 0, 2: 1}, []), (2, 3, {0: 0}, []), (3, 4, {0: 0, 5: 6}, []),
                                    (4, 5, {0: 0}, [])]),
        _case("cycle", [(0, 1, {0: 1}, []), (1, 2, {1: 2}, []), (2, 0, {2: 0}, [])]),
        _case("same_edge_twice_and_both_directions", [(0, 1, {3: 4}, []), (0, 1, {3: 4}, []), (1, 0, {4: 3}, [])]),
        # rows 0 and 1 of frame 0 both go to row 0 of frame 1: the chain hanging on it through frames 2..5 is dropped with it;
        # the 2-view track (2,4)-(3,4) next to it survives
        _case("many_to_one_drops_the_chain", [(0, 1, {0: 0, 1: 0}, [])] + chain[1:] + [(2, 3, {4: 4}, [])]),
        # every pair is one-to-one; frame 0 comes in twice only through frames 2 and 1
        _case("conflict_through_a_third_frame", [(0, 2, {0: 0}, []), (2, 1, {0: 0}, []), (1, 0, {0: 1}, [])]),
        _case("isolated_nodes_only", [(0, 1, {}, [])]),
        # min_views = 3: the 2-view components are SHORT and counted in totals[3], the 3-view one stays a track
        _case("min_views_3", [(0, 1, {0: 0, 1: 1}, []), (1, 2, {0: 0}, []), (3, 4, {2: 2}, [])], min_views=3),
        # idx1 of -1, counts[t], cap and INT32_MAX drop the row; counts[t] - 1 is the last valid one
        _case("idx1_out_of_range", [(0, 1, {0: -1, 1: 5, 2: CAP, 3: INT32_MAX, 4: 4}, [])], counts=[8, 5, 8, 8, 8, 8]),
        # a query row at counts[q] is ignored, the one at counts[q] - 1 is read
        _case("query_row_at_the_count", [(0, 1, {3: 3, 2: 2}, [])], counts=[3, 8, 8, 8, 8, 8]),
        # counts -3 -> 0 and cap + 5 -> cap; frame 3 holds nothing: nothing links into frames 0 and 3 or out of them
        _case("clamped_and_empty_counts", [(1, 2, {7: 7}, []), (0, 2, {0: 1}, []), (2, 0, {1: 0}, []), (2, 3, {2: 0}, []),
                                           (3, 4, {0: 0}, []), (4, 5, {6: 6}, [])], counts=[-3, CAP + 5, 8, 0, 8, 8]),
        _case("pair_index_out_of_range", [(6, 1, {0: 0}, []), (-1, 2, {0: 0}, []), (1, 7, {1: 1}, []), (3, INT32_MAX, {1: 1}, []),
                                          (4, 5, {1: 1}, [])]),
        _case("pair_of_a_frame_with_itself", [(2, 2, {0: 1}, []), (2, 3, {5: 5}, [])]),
        # the inlier byte 0 sits on the row that would join the two 2-view tracks into one 4-view track
        _case("inlier_zero_keeps_two_tracks_apart", [(0, 1, {0: 0}, []), (2, 3, {0: 0}, []), (1, 2, {0: 0}, [0])]),
    ]


def chain(order="forward", seed=0):
    """300 frames x 4 rows, row r of frame f matched to row r of frame f + 1: four tracks of 300 views."""
    n_frames, cap = 300, 4
    pq = np.arange(n_frames - 1, dtype=np.int32)
    if order == "reversed":
        pq = pq[::-1].copy()
    elif order == "shuffled":
        pq = np.random.default_rng(seed).permutation(pq).astype(np.int32)
    idx1 = np.tile(np.arange(cap, dtype=np.int32), (n_frames - 1, 1))
    return dict(name="chain_" + order, n_frames=n_frames, cap=cap, kps=make_kps(n_frames, cap, 12), counts=np.full(n_frames, cap, np.int32),
                pair_q=pq, pair_t=pq + 1, idx1=idx1, inlier=np.ones((n_frames - 1, cap), np.uint8), min_views=2)


def hub(conflict=False):
    """257 frames x 2 rows, row 0 of every frame 1..256 matched to row 0 of frame 0; conflict: frame 5 sends both rows there."""
    n_frames, cap = 257, 2
    pq = np.arange(1, n_frames, dtype=np.int32)
    idx1 = np.full((n_frames - 1, cap), -1, np.int32)
    idx1[:, 0] = 0
    if conflict:
        idx1[4, 1] = 0  # pair 4 is (5, 0)
    return dict(name="hub_conflict" if conflict else "hub", n_frames=n_frames, cap=cap, kps=make_kps(n_frames, cap, 13),
                counts=np.full(n_frames, cap, np.int32), pair_q=pq, pair_t=np.zeros(n_frames - 1, np.int32), idx1=idx1,
                inlier=np.ones((n_frames - 1, cap), np.uint8), min_views=2)


def random_windows(n_frames=40, cap=64, n_points=120, seed=5, wrong=0.03, neighbours=3):
    """Ground-truth points each seen in a window of 2..9 consecutive frames at a random free row; every frame paired with its
    next `neighbours`; the share `wrong` of the matched rows redirected to a random row, which creates conflicts."""
    rng = np.random.default_rng(seed)
    row_of = -np.ones((n_points, n_frames), np.int64)
    free = [list(rng.permutation(cap)) for _ in range(n_frames)]
    for p in range(n_points):
        length = int(rng.integers(2, 10))
        first = int(rng.integers(0, n_frames - length + 1))
        for f in range(first, first + length):
            row_of[p, f] = free[f].pop()
    pairs = [(f, f + d) for f in range(n_frames) for d in range(1, neighbours + 1) if f + d < n_frames]
    idx1 = np.full((len(pairs), cap), -1, np.int32)
    for k, (q, t) in enumerate(pairs):
        both = np.flatnonzero((row_of[:, q] >= 0) & (row_of[:, t] >= 0))
        idx1[k, row_of[both, q]] = row_of[both, t]
    matched = np.argwhere(idx1 >= 0)
    for k, i in matched[rng.random(len(matched)) < wrong]:
        idx1[k, i] = rng.integers(0, cap)
    inlier = (rng.random(idx1.shape) >= 0.02).astype(np.uint8)
    return dict(name="random_windows", n_frames=n_frames, cap=cap, kps=make_kps(n_frames, cap, seed + 1),
                counts=np.full(n_frames, cap, np.int32), pair_q=np.array([p[0] for p in pairs], np.int32),
                pair_t=np.array([p[1] for p in pairs], np.int32), idx1=idx1, inlier=inlier, min_views=2)


def restate(c, use_inlier=True, min_views=None):
    """tests/track_link_restate.py on a case -> its dict of lists."""
    return lr.link(c["kps"][..., :2], c["counts"].tolist(), c["n_frames"], c["cap"], c["pair_q"].tolist(), c["pair_t"].tolist(),
                   c["idx1"].reshape(-1).tolist(), c["inlier"].reshape(-1).tolist() if use_inlier else None, INTRINSICS,
                   c["min_views"] if min_views is None else min_views)


@functools.lru_cache(maxsize=None)
def random_case():
    """The random case and its restatement (with the inlier bytes and without), computed once per session and left unchanged."""
    c = random_windows()
    return c, restate(c, True), restate(c, False)


def as_arrays(e, N):
    """The restatement's lists as the arrays the device writes."""
    return dict(node_point=np.array(e["node_point"], np.int32).reshape(N), obs_cam=np.array(e["obs_cam"], np.int32).reshape(N),
                obs_point=np.array(e["obs_point"], np.int32).reshape(N), obs_xy=np.array(e["obs_xy"], np.float64).reshape(N, 2),
                obs_node=np.array(e["obs_node"], np.int32).reshape(N), point_len=np.array(e["point_len"], np.int32).reshape(N // 2),
                totals=np.array(e["totals"], np.int32))
