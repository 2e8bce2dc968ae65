"""Inputs for gh_merge_points_dev: a hand-built census on 6 frames x 8 rows, a pair of points whose verdict a fused multiply-add
would change, a hub (257 points joined on one root), a chain (300 points joined one to the next), random soups at the workgroup
boundaries, a random map whose long tracks were cut in two, and the synthetic scene of localize_cases with map points split.
tests/test_track_merge_cpu.py shows what they reach; tests/test_track_merge_gpu.py holds the device to
tests/track_merge_restate.py on them, byte for byte."""
import functools
import math
from fractions import Fraction

import numpy as np

import localize_cases as loc
import track_extend_cases as ec
import track_link_cases as lc
import track_link_restate as lr
import track_merge_restate as mr

INT32_MAX = 2**31 - 1
OUTPUTS = ("point_remap", "point_state", "point_select", "node_point", "obs_point", "point_len", "totals")
DTYPE = dict(point_remap=np.int32, point_state=np.uint8, point_select=np.uint8, node_point=np.int32, obs_point=np.int32,
             point_len=np.int32, totals=np.int32)
reorder = ec.reorder


def obs_of(node_point, counts, cap, n_points):
    """The obs_point array of gh_extend_tracks_dev for a map: the ids of the existing nodes that hold one, in ascending node id,
    padded with -1 to N."""
    N = len(node_point)
    ids = [int(node_point[n]) for n in mr.existing(counts, len(counts), cap) if 0 <= node_point[n] < n_points]
    return np.array(ids + [-1] * (N - len(ids)), np.int32)


def _case(name, n_frames, cap, counts, pairs, node_point, n_points, status=None, xyz=None, max_dist=1.0):
    counts = np.array(counts, np.int32)
    node_point = np.asarray(node_point, np.int32).reshape(-1)
    return dict(name=name, n_frames=n_frames, cap=cap, counts=counts, node_point=node_point, n_points=n_points,
                status=np.zeros(n_points, np.int32) if status is None else np.asarray(status, np.int32),
                xyz=np.zeros((n_points, 3)) if xyz is None else np.asarray(xyz, np.float64), max_dist=float(max_dist),
                obs_point=obs_of(node_point, counts, cap, n_points), **pairs)


CENSUS_MAX_DIST = 5.0
CENSUS_BEYOND = 2.0 ** -24  # (3 * 3 + 4 * 4) + CENSUS_BEYOND ** 2 is the double after 25: its square is one ulp of 25


def census():
    """n_points = 26, max_dist = 5, every point at the origin unless said otherwise; frame 5 has 6 rows.
      A  points 0, 1     (0,0)-(1,0) HOLDER-HOLDER; point 1 at (3, 4, 0): exactly max_dist, MERGED.  (2,0)-(0,0) both hold point 0:
                         the edge links nothing.  The row (5,6) does not exist and "holds" point 1: its entry is renamed like any
                         other, but it counts in nothing.
      B  points 2, 3     (0,1) and (2,1) joined only through the BRIDGE (1,1), which holds -1: MERGED, apart with bridge = 0.
      C  points 4, 5, 6  (0,2)-(1,2)-(2,2): a group of three, MERGED.
      D  points 7, 8     7 at (3,0) (4,0), 8 at (3,1); (4,0)-(3,1): both in frame 3, CONFLICT.
      E  points 9, 10    9 at (3,2) AND (3,3) -- a duplicate the map already had -- 10 at (4,2); (4,2)-(3,2): CONFLICT.
      F  points 11, 12   (0,5)-(1,5); point 12 at (100, 0, 0): FAR.
      G  points 13, 14   (4,3)-(2,3); point 14 at (3, 4, 2^-24): d2 is the double after 25, one ulp beyond, FAR.
      H  points 15, 16   (4,4)-(2,4); point 16 has a NaN coordinate: FAR.
      I  points 17 .. 19 18 at (0,6), 17 at (1,6), 19 at (2,6), (0,6)-(1,6)-(2,6); point 17 is not GH_TRACK_OK, so its node is
                         OUT and 18, 19 stay apart; without the status array the three are one MERGED group.
      J  points 20, 21   (0,7) - (5,1) [-4] - (4,5) [n_points] - (3,5) [INT32_MAX] - (1,7): joined through three BRIDGE nodes
                         whose codes are no ids; apart with bridge = 0.
      K  points 22, 23   (3,7)-(2,7) with the inlier byte 0: apart; MERGED without the inlier bytes.
      L  point 24        (4,6) matched to the row (5,6) that does not exist: the edge is dropped.  Point 25 is nowhere."""
    F, cap, n_points = 6, 8, 26
    node_point = np.full((F, cap), -1, np.int32)
    held = {(0, 0): 0, (2, 0): 0, (1, 0): 1, (0, 1): 2, (2, 1): 3, (0, 2): 4, (1, 2): 5, (2, 2): 6, (3, 0): 7, (4, 0): 7, (3, 1): 8,
            (3, 2): 9, (3, 3): 9, (4, 2): 10, (0, 5): 11, (1, 5): 12, (2, 3): 13, (4, 3): 14, (2, 4): 15, (4, 4): 16, (1, 6): 17,
            (0, 6): 18, (2, 6): 19, (0, 7): 20, (1, 7): 21, (2, 7): 22, (3, 7): 23, (4, 6): 24, (5, 6): 1, (5, 1): -4,
            (4, 5): n_points, (3, 5): INT32_MAX}
    for (f, i), v in held.items():
        node_point[f, i] = v
    pairs = [(0, 1, {0: 0, 2: 2, 5: 5, 6: 6}, []), (1, 0, {1: 1}, []), (1, 2, {1: 1, 2: 2, 6: 6}, []), (2, 0, {0: 0}, []),
             (4, 3, {0: 1, 2: 2, 5: 5}, []), (4, 2, {3: 3, 4: 4}, []), (5, 0, {1: 7}, []), (5, 4, {1: 5}, []), (3, 1, {5: 7}, []),
             (3, 2, {7: 7}, [7]), (4, 5, {6: 6}, [])]
    status = np.zeros(n_points, np.int32)
    status[17] = 3
    xyz = np.zeros((n_points, 3))
    xyz[1] = (3.0, 4.0, 0.0)
    xyz[12] = (100.0, 0.0, 0.0)
    xyz[14] = (3.0, 4.0, CENSUS_BEYOND)
    xyz[16] = (float("nan"), 0.0, 0.0)
    return _case("census", F, cap, [8, 8, 8, 8, 8, 6], ec._pairs(pairs, cap), node_point, n_points, status, xyz, CENSUS_MAX_DIST)


def exact_d2(a, b):
    return sum((Fraction(x) - Fraction(y)) ** 2 for x, y in zip(a, b))


def fused_d2(a, b):
    """(fma(dx, dx, dy * dy)) + dz * dz: what a compiler that contracts dx * dx + dy * dy would evaluate.  The fused operation
    rounds the exact dx * dx + round(dy * dy) once; Fraction gives that exact value and float() rounds it to nearest even."""
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return float(Fraction(dx) * Fraction(dx) + Fraction(dy * dy)) + dz * dz


@functools.lru_cache(maxsize=None)
def fused_pair(seed=1):
    """Two points and a max_dist at which the contract's evaluation and the fused one give different verdicts: a seeded search.
    -> (a, b, max_dist, contract d2, fused d2)."""
    rng = np.random.default_rng(seed)
    for _ in range(100000):
        a, b = tuple(rng.uniform(-2.0, 2.0, 3).tolist()), tuple(rng.uniform(-2.0, 2.0, 3).tolist())
        plain, fused = mr.d2(a, b), fused_d2(a, b)
        if plain == fused:
            continue
        lo, hi = min(plain, fused), max(plain, fused)
        m = math.sqrt(lo)
        for cand in (m, math.nextafter(m, 4.0), math.nextafter(m, 0.0)):  # a max_dist whose square separates the two
            if lo <= cand * cand < hi:
                return a, b, cand, plain, fused
    raise AssertionError("no pair found")


def fused():
    """Two points in two frames, matched: the gate decides, and a fused multiply-add would decide the other way."""
    a, b, max_dist, _, _ = fused_pair()
    pairs = ec._pairs([(1, 0, {0: 0}, [])], 2)
    return _case("fused", 2, 2, [2, 2], pairs, [0, -1, 1, -1], 2, None, [a, b], max_dist)


def hub(conflict=False):
    """257 frames x 2 rows, point f held at row 0 of frame f, every frame 1 .. 256 matched to frame 0: one group of 257 points,
    256 unions on one root.  conflict: frame 5 also holds point 9 at row 1."""
    F, cap = 257, 2
    node_point = np.full((F, cap), -1, np.int32)
    node_point[:, 0] = np.arange(F)
    if conflict:
        node_point[5, 1] = 9
    idx1 = np.full((F - 1, cap), -1, np.int32)
    idx1[:, 0] = 0
    pairs = dict(pair_q=np.arange(1, F, dtype=np.int32), pair_t=np.zeros(F - 1, np.int32), idx1=idx1, inlier=np.ones((F - 1, cap), np.uint8))
    return _case("hub_conflict" if conflict else "hub", F, cap, [cap] * F, pairs, node_point, F)


def chain():
    """300 points, point p held at row 0 of the frames 2p and 2p + 1, frame 2p + 1 matched to frame 2p + 2: the points are joined
    p - (p + 1), the longest paths a union-find can see.  Row 1 of every frame holds nothing and is matched to nothing."""
    P, cap = 300, 2
    F = 2 * P
    node_point = np.full((F, cap), -1, np.int32)
    node_point[:, 0] = np.arange(F) // 2
    idx1 = np.full((P - 1, cap), -1, np.int32)
    idx1[:, 0] = 0
    q = 2 * np.arange(P - 1, dtype=np.int32) + 1
    pairs = dict(pair_q=q, pair_t=q + 1, idx1=idx1, inlier=np.ones((P - 1, cap), np.uint8))
    return _case("chain", F, cap, [cap] * F, pairs, node_point, P)


def soup(n_frames, cap, counts, n_points, seed):
    """Random everything, valid or not: node_point from the ids and from values the contract must turn down, a tenth of the
    points not GH_TRACK_OK, coordinates on a small integer grid (so the gate of max_dist = 2 goes both ways) with a few NaN,
    idx1 from -1 .. cap.  The first and the last existing node hold a point, and the last point id is held."""
    rng = np.random.default_rng(seed)
    N = n_frames * cap
    bad = np.array([-1, -1, -1, -2, -3, -4, n_points, INT32_MAX, -INT32_MAX - 1], np.int64)
    node_point = np.where(rng.random(N) < 0.55, rng.integers(0, n_points, N), bad[rng.integers(0, len(bad), N)])
    counts = np.array(counts, np.int32)
    node_point[0], node_point[(n_frames - 1) * cap + int(counts[-1]) - 1] = n_points - 1, 0
    pairs = [(f, f + d) for f in range(n_frames) for d in (1, 2) if f + d < n_frames] + [(n_frames - 1, 0), (1, 1), (n_frames, 0)]
    idx1 = np.where(rng.random((len(pairs), cap)) < 0.12, rng.integers(-1, cap + 1, (len(pairs), cap)), -1).astype(np.int32)
    inlier = (rng.random(idx1.shape) >= 0.1).astype(np.uint8)
    status = np.where(rng.random(n_points) < 0.1, rng.integers(1, 6, n_points), 0).astype(np.int32)
    xyz = rng.integers(0, 2, (n_points, 3)).astype(np.float64)
    xyz[rng.random(n_points) < 0.02, 1] = np.nan
    return _case("soup_%dx%d" % (n_frames, cap), n_frames, cap, counts,
                 dict(pair_q=np.array([p[0] for p in pairs], np.int32), pair_t=np.array([p[1] for p in pairs], np.int32), idx1=idx1,
                      inlier=inlier), node_point, n_points, status, xyz, 1.25)


def boundaries():
    """N = 512 with n_points = 257 (the points one lane into their second workgroup, the n_points + N = 769 elements one lane into
    their fourth) and N = 513 with n_points = 256 (the points fill one workgroup exactly, the nodes are one lane into their
    third)."""
    return [soup(8, 64, [64] * 8, 257, 7), soup(3, 171, [171, 171, 170], 256, 8)]


def split_tracks(node_point, counts, cap, n_points, which):
    """The later half (in node order) of the existing nodes of every point in `which` gets a new id; the new ids go on after
    n_points in the order of `which`.  -> (node_point, {new id: old id})."""
    out = np.array(node_point, np.int32).copy()
    exists = set(mr.existing(counts, len(counts), cap))
    new_of = {}
    for k, p in enumerate(which):
        nodes = [n for n in np.flatnonzero(out == p).tolist() if n in exists]
        out[nodes[len(nodes) // 2:]] = n_points + k
        new_of[n_points + k] = int(p)
    return out, new_of


def random_split(seed=5, far_every=7):
    """track_link_cases.random_windows without wrong matches linked by the restated link: the map.  Every track of at least 4
    views is cut into two ids with equal coordinates plus noise of 1e-3, and every far_every-th of them is moved 10 away;
    max_dist = 0.1.  The call gets the matches of the same windows with 3 % of them wrong and 2 % of the inlier bytes 0: every
    cut is shown by the edges across it, and a wrong match joins two tracks that are different points -- a CONFLICT where they
    share a frame, FAR where they do not."""
    clean = lc.random_windows(n_frames=40, cap=64, n_points=160, seed=seed, wrong=0.0)
    c = lc.random_windows(n_frames=40, cap=64, n_points=160, seed=seed)
    m = lr.link(c["kps"][..., :2], c["counts"].tolist(), c["n_frames"], c["cap"], c["pair_q"].tolist(), c["pair_t"].tolist(),
                clean["idx1"].reshape(-1).tolist(), None, lc.INTRINSICS, 2)
    n_old = m["totals"][1]
    which = [p for p in range(n_old) if m["point_len"][p] >= 4]
    node_point, new_of = split_tracks(m["node_point"], c["counts"], c["cap"], n_old, which)
    rng = np.random.default_rng(seed + 50)
    n_points = n_old + len(which)
    xyz = np.zeros((n_points, 3))
    xyz[:n_old] = rng.uniform(-5.0, 5.0, (n_old, 3))
    for k, (new, old) in enumerate(sorted(new_of.items())):
        xyz[new] = xyz[old] + rng.normal(0.0, 1e-3, 3) + (10.0 if k % far_every == 0 else 0.0)
    pairs = dict(pair_q=c["pair_q"], pair_t=c["pair_t"], idx1=c["idx1"], inlier=c["inlier"])
    return _case("random_split", c["n_frames"], c["cap"], c["counts"], pairs, node_point, n_points, None, xyz, 0.1)


def restate(c, use_inlier=True, use_status=True, use_gate=True, bridge=1, use_obs=True):
    """tests/track_merge_restate.py on a case -> its dict of lists."""
    return mr.merge(c["counts"].tolist(), c["n_frames"], c["cap"], c["pair_q"].tolist(), c["pair_t"].tolist(),
                    c["idx1"].reshape(-1).tolist(), c["inlier"].reshape(-1).tolist() if use_inlier else None, c["node_point"].tolist(),
                    c["n_points"], c["status"].tolist() if use_status else None, [tuple(r) for r in c["xyz"].tolist()] if use_gate else None,
                    c["max_dist"], bridge, c["obs_point"].tolist() if use_obs else None)


@functools.lru_cache(maxsize=None)
def random_case():
    """The random case and its restatement, computed once per session and left unchanged."""
    c = random_split()
    return c, restate(c)


def as_arrays(e):
    """The restatement's lists as the arrays the device writes (obs_point: None when there is none)."""
    return {k: (None if e[k] is None else np.array(e[k], DTYPE[k])) for k in OUTPUTS}


SCENE_SPLIT = 12


@functools.lru_cache(maxsize=None)
def scene_split():
    """localize_cases.scene(): its map (the restated link on the map pairs, which the device's link equals byte for byte) and the
    same map with SCENE_SPLIT of its points of at least 4 observations split in two as tools/track_merge_probe.py splits them:
    the later half of a point's nodes gets an id above all others.  -> the scene's dict plus n_points (the capacity N // 2),
    n_used, node_point / obs_point (unsplit), node_point_split / obs_point_split, split {new id: old id}, and the link's obs_cam /
    obs_xy (which a split leaves as they are)."""
    s = loc.scene()
    F, cap = s["n_frames"], s["cap"]
    N = F * cap
    m = lr.link(s["kps"][..., :2], s["counts"].tolist(), F, cap, s["map_q"].tolist(), s["map_t"].tolist(),
                s["map_idx1"].reshape(-1).tolist(), None, s["intrinsics"], 2)
    n_used = m["totals"][1]
    long = [p for p in range(n_used) if m["point_len"][p] >= 4]
    which = long[::max(1, len(long) // SCENE_SPLIT)][:SCENE_SPLIT]
    assert len(which) >= 8 and n_used + len(which) <= N // 2
    node_point = np.array(m["node_point"], np.int32)
    split, new_of = split_tracks(node_point, s["counts"], cap, n_used, which)
    return dict(s, n_points=N // 2, n_used=n_used, node_point=node_point, obs_point=np.array(m["obs_point"], np.int32),
                node_point_split=split, obs_point_split=obs_of(split, s["counts"], cap, N // 2), split=new_of,
                obs_cam=np.array(m["obs_cam"], np.int32), obs_xy=np.array(m["obs_xy"], np.float64))
