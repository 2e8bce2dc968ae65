"""One input each for gh_link_tracks_dev, gh_extend_tracks_dev and gh_pnp_gather_pairs_dev with more than 1024 * 256 nodes: the
*_flags kernels run at most 1024 workgroups of 256 lanes, so from node 262144 on every workgroup takes a SECOND trip through
its loop before it adds up its counters.  259 frames x 1024 rows, N = 265216: the frames 256, 257 and 258 lie past node 262144.
counts is zero except in three low frames (0, 1, 2; localize: 3 as well) and in those three high frames, 40 rows each, so the
plain-Python restatements stay quick.  The same pattern of rows is laid on the low group and on the high group: every verdict
occurs in both, and in the high group its LABEL (the smallest node of the component, where the verdict is counted) lies past
node 262144 too.  tests/test_*_cpu.py show what the restatements reach on these inputs; the GPU census tests hold the device to
them, byte for byte."""
import functools

import numpy as np

import localize_cases as loc
import track_extend_cases as ec
import track_link_cases as lc

N_FRAMES, CAP, ROWS = 259, 1024, 40
LOW, HIGH = (0, 1, 2), (256, 257, 258)
SECOND_TRIP = 1024 * 256  # the first node of the second trip
assert HIGH[0] * CAP >= SECOND_TRIP and N_FRAMES * CAP + 1 <= 2 * SECOND_TRIP


def _counts(live):
    counts = np.zeros(N_FRAMES, np.int32)
    counts[list(live)] = ROWS
    return counts


def _pair_arrays(pairs, keep_name):
    """pairs: [(q, t, {row: idx1}, [rows whose inlier / keep byte is 0])]; rows not listed hold idx1 = -1, byte = 1."""
    idx1 = np.full((len(pairs), CAP), -1, np.int32)
    keep = np.ones((len(pairs), CAP), np.uint8)
    for p, (_, _, rows, off) in enumerate(pairs):
        for i, j in rows.items():
            idx1[p, i] = j
        for i in off:
            keep[p, i] = 0
    return {"pair_q": np.array([p[0] for p in pairs], np.int32), "pair_t": np.array([p[1] for p in pairs], np.int32), "idx1": idx1,
            keep_name: keep}


def _link_pairs():
    """On each group (A, B, C): rows 0 .. 9 chained A-B-C (ten tracks of three views); rows 10 .. 14 matched A-B only (a track
    for min_views = 2, SHORT of two nodes for 3), row 12 goes on to C under an inlier byte 0; rows 20 and 21 of B both go to row 20
    of A (CONFLICT).  Rows 30 .. 34 of frame 2 are matched to the same rows of frame 256 and row 35 of frame 258 to row 35 of
    frame 0: tracks with the label in a low frame and an observation past node 262144.  Every other row stays alone."""
    pairs = []
    for A, B, C in (LOW, HIGH):
        pairs += [(A, B, {r: r for r in range(15)}, []), (B, C, {**{r: r for r in range(10)}, 12: 12}, [12]), (B, A, {20: 20, 21: 20}, [])]
    return pairs + [(LOW[2], HIGH[0], {r: r for r in range(30, 35)}, []), (HIGH[2], LOW[0], {35: 35}, [])]


@functools.lru_cache(maxsize=None)
def link_case():
    return dict(name="wide_link", n_frames=N_FRAMES, cap=CAP, kps=lc.make_kps(N_FRAMES, CAP, 41), counts=_counts(LOW + HIGH), min_views=2,
                **_pair_arrays(_link_pairs(), "inlier"))


@functools.lru_cache(maxsize=None)
def link_restated(use_inlier=True, min_views=2):
    return lc.restate(link_case(), use_inlier, min_views)


@functools.lru_cache(maxsize=None)
def extend_case():
    """The pairs of link_case() on the rows 0 .. 35, which are FREE.  n_points = 6.  Rows 36 .. 39: frame 0 holds the points
    0, 1, 2, 3 and frame 1 the points 0, 1 (MAPPED).  (2,36) and (256,36) claim point 0: ADOPTED.  (2,37) (2,38) both claim point 4,
    (257,36) (257,37) both claim point 1: REJECTED.  (258,38) holds point 2 already, so (258,36), which claims it, is REJECTED;
    (258,37) claims point 3 with row_inlier 0: FREE."""
    n_points = 6
    node_point = np.full((N_FRAMES, CAP), -1, np.int32)
    node_point[0, 36:40] = [0, 1, 2, 3]
    node_point[1, 36:38] = [0, 1]
    node_point[258, 38] = 2
    row_point = np.full((N_FRAMES, CAP), -1, np.int32)
    row_inlier = np.zeros((N_FRAMES, CAP), np.uint8)
    claims = {(2, 36): (0, 1), (256, 36): (0, 1), (2, 37): (4, 1), (2, 38): (4, 1), (257, 36): (1, 1), (257, 37): (1, 1), (258, 36): (2, 1),
              (258, 37): (3, 0)}
    for (f, i), (c, b) in claims.items():
        row_point[f, i], row_inlier[f, i] = c, b
    return dict(name="wide_extend", n_frames=N_FRAMES, cap=CAP, kps=lc.make_kps(N_FRAMES, CAP, 42), counts=_counts(LOW + HIGH),
                node_point=node_point.reshape(-1), n_points=n_points, row_point=row_point.reshape(-1), row_inlier=row_inlier.reshape(-1),
                min_views=3, **_pair_arrays(_link_pairs(), "inlier"))


@functools.lru_cache(maxsize=None)
def extend_restated(use_inlier=True, use_map=True, use_claims=True, min_views=3):
    return ec.restate(extend_case(), use_inlier, use_map, use_claims, min_views)


@functools.lru_cache(maxsize=None)
def localize_case():
    """The frames 0, 1, 2 hold the map of 40 points: frames 0 and 1 see point r at row r, frame 2 sees point 39 - r there; point 5
    is not GH_TRACK_OK.  The query frames 3, 256, 257 and 258 are each matched to the three of them: rows 0 .. 19 see their own
    point in frame 0, rows 0 .. 9 again in frame 1 and row 12 in frame 2 (row 27 there): correspondences.  Row 10 sees point 11
    in frame 1: AMBIGUOUS.  Row 20 sees point 15, as row 15 does: both SHARED.  Row 16 sees point 17 in frame 1 under a keep byte 0."""
    n_points = 40
    node_point = np.full((N_FRAMES, CAP), -1, np.int32)
    node_point[0, :ROWS] = node_point[1, :ROWS] = np.arange(ROWS)
    node_point[2, :ROWS] = np.arange(ROWS)[::-1]
    pairs = []
    for Q in (3,) + HIGH:
        pairs += [(Q, 0, {**{r: r for r in range(20)}, 20: 15}, []), (Q, 1, {**{r: r for r in range(10)}, 10: 11, 16: 17}, [16]),
                  (Q, 2, {12: 27}, [])]
    status = np.zeros(n_points, np.int32)
    status[5] = 1
    return dict(name="wide_localize", n_frames=N_FRAMES, cap=CAP, kps=loc.make_kps(N_FRAMES, CAP, 43), counts=_counts(LOW + (3,) + HIGH),
                node_point=node_point.reshape(-1), point_xyz=loc.make_points(n_points, 44), status=status, **_pair_arrays(pairs, "keep"))


@functools.lru_cache(maxsize=None)
def localize_restated(use_keep=True, use_status=True):
    return loc.restate(localize_case(), use_keep, use_status)
