"""Inputs for gh_search_projection_dev, shared by tests/test_search_projection_cpu.py (what they reach: its census) and
tests/test_search_projection_gpu.py (the device against tests/search_projection_restate.py).  A case is a dict of host arrays:
kps (n_frames x cap x 7 float32 view of the KeyPoint records, the octave as int32 bits in column 5), desc (n_frames x cap x 32
uint8), counts, poses (n_frames x 7 T_wc), frame_search (uint8), node_point / row_point (int32 N) and row_inlier (uint8 N),
n_points, xyz, status (int32), select (uint8), the four summaries views / point_desc / normal / dist, intrinsics, size and params
(a dict as search_projection_restate.DEFAULTS).

edges() and windows() are built by hand around cameras with the identity rotation, where the rotation of the contract returns
its argument exactly and a pixel with a dyadic offset from the principal point is hit exactly; soup() is seeded noise over
rotated cameras with everything a map can hold."""
import functools

import numpy as np

import search_projection_restate as sr

OUTPUTS = ("row_point", "row_inlier", "row_dist", "frame_totals", "totals")
DTYPE = dict(row_point=np.int32, row_inlier=np.uint8, row_dist=np.uint16, frame_totals=np.int32, totals=np.int32)
INTRINSICS = (500.0, 500.0, 320.0, 240.0)
SIZE = (640, 480)
I32_MIN, I32_MAX = -2**31, 2**31 - 1
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
NAN, INF = float("nan"), float("inf")


def _flip(rng, base, k):
    """`base` (32 bytes) with k distinct bits flipped."""
    d = base.copy()
    for bit in rng.choice(256, size=k, replace=False):
        d[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return d


def _f32_below(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def _f32_above(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


class _Build:
    """Points and keypoints one by one.  A point is placed through the pixel it should have in a frame; the pixel it really has
    comes from the restatement's projection, and keypoints are placed relative to that."""

    def __init__(self, name, n_frames, cap, seed, params=None, poses=None):
        self.name, self.F, self.cap = name, n_frames, cap
        self.rng = np.random.default_rng(seed)
        self.prm = dict(sr.DEFAULTS, **(params or {}))
        self.pw = sr.pow_table(self.prm["scale_factor"])
        self.poses = np.array(poses if poses is not None else [IDENTITY] * n_frames, np.float64)
        self.rows = [[] for _ in range(n_frames)]  # per frame: (x, y, octave, desc, node_point, row_point, row_inlier)
        self.points = []                           # (xyz, status, select, views, desc, normal, (min, max))
        self.counts = None
        self.frame_search = np.ones(n_frames, np.uint8)

    def back_project(self, f, u, v, z):
        """The world point at depth z behind pixel (u, v) of frame f (numpy: the placement need not be exact)."""
        fx, fy, cx, cy = INTRINSICS
        q, t = self.poses[f, :4], self.poses[f, 4:]
        Xc = [(u - cx) / fx * z, (v - cy) / fy * z, z]
        return [float(a + b) for a, b in zip(sr.quat_rotate(list(q), Xc), t)]

    def pixel(self, f, X):
        return sr.project(list(self.poses[f]), X, *INTRINSICS)[2]

    def point(self, X, f_ref=0, level=0, cos=1.0, views=2, status=0, select=1, desc=None, max_scale=0.99):
        """A point at X whose window in frame f_ref is at `level` and whose normal makes the cosine `cos` with the ray from
        f_ref: max_dist = max_scale * dist * pow[level] puts exactly `level` entries of the table below it.  -> its id."""
        d = np.array(X) - self.poses[f_ref, 4:]
        dist = float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))  # (the contract's order: max_scale = 1 is to the bit)
        ray = d / dist if dist > 0 else np.array([0.0, 0.0, 1.0])
        perp = np.cross(ray, [0.0, 1.0, 0.0])
        perp /= np.linalg.norm(perp)
        normal = cos * ray + np.sqrt(max(0.0, 1.0 - cos * cos)) * perp
        max_dist = max_scale * dist * self.pw[level]
        if desc is None:
            desc = self.rng.integers(0, 256, size=32, dtype=np.uint8)
        self.points.append((list(map(float, X)), status, select, views, desc, normal.tolist(),
                            (max_dist / self.pw[self.prm["n_levels"] - 1], max_dist)))
        return len(self.points) - 1

    def kp(self, f, x, y, octave, desc=None, node_point=-1, row_point=-1, row_inlier=0):
        if desc is None:
            desc = self.rng.integers(0, 256, size=32, dtype=np.uint8)
        self.rows[f].append((x, y, octave, desc, node_point, row_point, row_inlier))
        assert len(self.rows[f]) <= self.cap, (self.name, f, "too many keypoints")
        return len(self.rows[f]) - 1

    def near(self, p, flips):
        return _flip(self.rng, self.points[p][4], flips)

    def done(self, shuffle=False, **extra):
        F, cap = self.F, self.cap
        kps = np.zeros((F, cap, 7), np.float32)
        octave = np.zeros((F, cap), np.int32)
        desc = self.rng.integers(0, 256, size=(F, cap, 32), dtype=np.uint8)
        node_point = self.rng.choice([-1, -2, -3], size=(F, cap)).astype(np.int32)
        row_point = self.rng.choice([-1, -2, -3, -4], size=(F, cap)).astype(np.int32)
        row_inlier = np.zeros((F, cap), np.uint8)
        # what lies past a frame's count looks like rows: in-range points, inliers, coordinates in the image
        kps[..., 0] = self.rng.uniform(0, SIZE[0], size=(F, cap)).astype(np.float32)
        kps[..., 1] = self.rng.uniform(0, SIZE[1], size=(F, cap)).astype(np.float32)
        counts = np.zeros(F, np.int32)
        n_points = len(self.points)
        for f, rows in enumerate(self.rows):
            order = self.rng.permutation(len(rows)) if shuffle else np.arange(len(rows))
            for i, k in enumerate(order):
                x, y, o, d, npnt, rp, ri = rows[k]
                kps[f, i, 0], kps[f, i, 1], octave[f, i], desc[f, i] = x, y, o, d
                node_point[f, i], row_point[f, i], row_inlier[f, i] = npnt, rp, ri
            counts[f] = len(rows)
            if n_points:
                past = np.arange(len(rows), cap)
                node_point[f, past] = self.rng.integers(0, n_points, size=len(past))
                row_point[f, past] = self.rng.integers(0, n_points, size=len(past))
                row_inlier[f, past] = 1
        if self.counts is not None:
            for f, c in self.counts.items():  # (a count that says something else than the rows laid down)
                counts[f] = c
        kps[..., 5] = octave.view(np.float32)
        pts = self.points
        c = dict(name=self.name, n_frames=F, cap=cap, kps=kps, desc=desc, counts=counts, poses=self.poses,
                 frame_search=self.frame_search, node_point=node_point.reshape(-1), row_point=row_point.reshape(-1),
                 row_inlier=row_inlier.reshape(-1), n_points=n_points,
                 xyz=np.array([p[0] for p in pts], np.float64).reshape(n_points, 3),
                 status=np.array([p[1] for p in pts], np.int32), select=np.array([p[2] for p in pts], np.uint8),
                 views=np.array([p[3] for p in pts], np.int32),
                 point_desc=np.array([p[4] for p in pts], np.uint8).reshape(n_points, 32),
                 normal=np.array([p[5] for p in pts], np.float64).reshape(n_points, 3),
                 dist=np.array([p[6] for p in pts], np.float64).reshape(n_points, 2), intrinsics=INTRINSICS, size=SIZE,
                 params=self.prm)
        c.update(extra)
        return c


@functools.lru_cache(maxsize=None)
def edges():
    """Every gate on both sides of its bound, the strict window, and the poses that are not poses.  Frame 0: the identity at the
    origin, where everything is placed.  Frame 1: a NaN in the translation.  Frame 2: a NaN in the quaternion.  Frame 3: the
    identity, its centre on a point.  Frame 4: the identity at the origin with a count of 0.  Frame 5: not searched."""
    poses = [IDENTITY, (0, 0, 0, 1, NAN, 0, 0), (0, 0, NAN, 1, 0, 0, 0), (0, 0, 0, 1, 0.5, 0.25, 4.0), IDENTITY, IDENTITY]
    b = _Build("edges", 6, 64, seed=41, poses=poses)
    b.frame_search[5] = 0
    b.counts = {4: 0}
    tag = {}
    # the strict window: u = 382.5, v = 302.5 exactly (X = (0.5, 0.5, 4)), level 0; near: radius 2.5, far: radius 4
    for name, X, cos, radius in (("near", [0.5, 0.5, 4.0], 1.0, 2.5), ("far", [-0.5, -0.5, 4.0], 0.9, 4.0)):
        p = b.point(X, cos=cos)
        u, v = b.pixel(0, X)
        assert (u, v) == ((382.5, 302.5) if name == "near" else (257.5, 177.5))
        tag[name] = p
        for k, (dx, dy) in enumerate(((radius, 0.0), (-radius, 0.0), (0.0, radius), (0.0, -radius))):
            # exactly on the border (excluded), and one float inside it (included), each alone in its own copy of the point
            on = (u + dx, v + dy)
            inside = (_f32_below(on[0]) if dx > 0 else _f32_above(on[0]) if dx < 0 else on[0],
                      _f32_below(on[1]) if dy > 0 else _f32_above(on[1]) if dy < 0 else on[1])
            tag["%s_on_%d" % (name, k)] = (p, b.kp(0, on[0], on[1], 0, b.near(p, 3 + k)))
            tag["%s_in_%d" % (name, k)] = (p, b.kp(0, inside[0], inside[1], 0, b.near(p, 20 + 12 * k)))
    # the cosine on each side of near_cos and of min_view_cos, with a keypoint 3 pixels off: inside 4, outside 2.5
    for k, cos in enumerate((0.9985, 0.9975, 0.5005, 0.4995, -0.3)):
        X = b.back_project(0, 100.0 + 40.0 * k, 100.0, 5.0)
        p = b.point(X, cos=cos)
        u, v = b.pixel(0, X)
        tag["cos_%d" % k] = (p, b.kp(0, u + 3.0, v, 0, b.near(p, 10)))
    # the depth on each side of 1e-9 (on the axis: u = cx), the image on each side of each border
    tag["depth"] = [b.point([0.0, 0.0, z], views=1) for z in (1e-9, 2e-9, -1.0, 0.0)]
    tag["border"] = []
    for u, v in ((639.9, 200.0), (640.1, 200.0), (0.1, 200.0), (-0.1, 200.0), (300.0, 479.9), (300.0, 480.1), (300.0, 0.1), (300.0, -0.1)):
        tag["border"].append(b.point(b.back_project(0, u, v, 6.0)))
    # u just below the width: the last double below 640 that the projection reaches from this side
    z, x = 4.0, (640.0 - 320.0) / 500.0 * 4.0
    while b.pixel(0, [x, 0.0, z])[0] < 640.0:
        x = float(np.nextafter(x, 10.0))
    while b.pixel(0, [x, 0.0, z])[0] >= 640.0:
        x = float(np.nextafter(x, 0.0))
    tag["last_u"] = b.point([x, 0.0, z])
    tag["first_out_u"] = b.point([float(np.nextafter(x, 10.0)), 0.0, z])
    # the range on each side of both bounds: max_dist = dist / 1.2 and min_dist = dist / 0.8, a hair each way
    for k, scale in enumerate((1.0 / 1.2 * (1 + 1e-9), 1.0 / 1.2 * (1 - 1e-9))):
        tag["range_hi_%d" % k] = b.point(b.back_project(0, 420.0 + 30 * k, 400.0, 5.0), max_scale=scale)
    top = b.pw[b.prm["n_levels"] - 1]
    for k, scale in enumerate((top / 0.8 * (1 - 1e-9), top / 0.8 * (1 + 1e-9))):
        tag["range_lo_%d" % k] = b.point(b.back_project(0, 480.0 + 30 * k, 400.0, 5.0), max_scale=scale)
    # a point at the centre of frame 3; points that are not searchable
    tag["centre"] = b.point([0.5, 0.25, 4.0])
    tag["not_searchable"] = [b.point(b.back_project(0, 200.0, 300.0, 5.0), views=0), b.point(b.back_project(0, 210.0, 300.0, 5.0), status=3),
                             b.point(b.back_project(0, 220.0, 300.0, 5.0), select=0), b.point(b.back_project(0, 230.0, 300.0, 5.0), views=-2)]
    for p in tag["not_searchable"]:
        u, v = b.pixel(0, b.points[p][0])
        b.kp(0, u, v, 0, b.near(p, 0))
    # WEAK and RATIO on each side: h = 100 / 101 alone in the window; (h, second) = (40, 50) and (41, 50) at one octave, and
    # (41, 50) at two octaves (level 1: octaves 0 and 1 are both admitted)
    for k, (h1, h2, o2, lvl) in enumerate(((100, None, 0, 0), (101, None, 0, 0), (40, 50, 0, 0), (41, 50, 0, 0), (41, 50, 0, 1),
                                           (0, 0, 0, 0))):
        X = b.back_project(0, 60.0 + 50.0 * k, 420.0, 5.0)
        p = b.point(X, level=lvl)
        u, v = b.pixel(0, X)
        rows = [b.kp(0, u + 1.0, v, lvl, b.near(p, h1))]
        if h2 is not None:
            rows.append(b.kp(0, u - 1.0, v + 1.0, o2, b.near(p, h2)))
        tag["match_%d" % k] = (p, rows)
    # max_dist = dist * pow[k] to the bit: the count of the contract says level k, and where a logarithm says k + 1 (it rounds)
    # the keypoint at octave k - 1 tells the two apart
    tag["on_level"] = []
    for k in range(1, 8):
        for z in (3.0, 4.5, 5.0, 6.25, 7.0):
            X = b.back_project(0, 40.0 + 80.0 * k, 40.0, z)
            dd = float(np.sqrt((X[0] * X[0] + X[1] * X[1]) + X[2] * X[2]))
            if int(np.ceil(np.log(dd * b.pw[k] / dd) / np.log(1.2))) == k + 1 and len(tag["on_level"]) < 3:
                p = b.point(X, level=k, max_scale=1.0)
                u, v = b.pixel(0, X)
                tag["on_level"].append((p, k, b.kp(0, u + 1.0, v, k - 1, b.near(p, 9))))
                break
    assert tag["on_level"]
    return b.done(tag=tag)


@functools.lru_cache(maxsize=None)
def windows():
    """radius_scale = 5: windows over 1, 2 and many cells, over every border, with 1, 8, 9 and 70 candidates, identical
    descriptors, TAKEN nodes and keypoints whose coordinates are not in the image or not numbers.  One frame with the identity
    at the origin (frame 0), one that is not searched, one searched frame with a negative count."""
    b = _Build("windows", 3, 256, seed=42, params=dict(radius_scale=5.0))
    b.frame_search[1] = 0
    b.counts = {2: -7}
    tag = {"crowd": {}}
    other = b.point([0.0, 0.0, -5.0])  # the point of the TAKEN nodes: HELD in frame 0, behind it
    # crowds: n candidates in a window at level 7 (radius 5 * 2.5 * 1.2^7 = 44.8: four or more cells of 32 pixels each way)
    for k, n in enumerate((1, 8, 9, 70)):
        X = b.back_project(0, 120.0 + 130.0 * k, 140.0, 4.0 + k)
        p = b.point(X, level=7)
        u, v = b.pixel(0, X)
        hs = b.rng.permutation([30] + list(range(60, 60 + 2 * (n - 1), 2)))  # distinct distances, a far second: no RATIO
        rows = [b.kp(0, u + float(b.rng.uniform(-40, 40)), v + float(b.rng.uniform(-40, 40)), 7 - int(j % 2), b.near(p, int(h)))
                for j, h in enumerate(hs)]
        tag["crowd"][n] = (p, rows)
        b.kp(0, u + 1.0, v + 1.0, 5, b.near(p, 0))   # the right place, the wrong octave
        b.kp(0, u - 2.0, v + 1.0, 8, b.near(p, 0))
        b.kp(0, u, v, 7, b.near(p, 0), node_point=other if n == 8 else -1, row_point=other, row_inlier=1)  # TAKEN by another point
    # one cell, two cells: level 0 near (radius 12.5) in the middle of a cell and across a cell border
    for name, (u0, v0) in (("one_cell", (336.0, 304.0)), ("two_cells", (352.0, 368.0)), ("two_cells_y", (400.0, 320.0))):
        X = b.back_project(0, u0, v0, 5.0)
        p = b.point(X)
        u, v = b.pixel(0, X)
        tag[name] = (p, [b.kp(0, u - 9.0, v - 9.0, 0, b.near(p, 12)), b.kp(0, u + 9.0, v + 9.0, 0, b.near(p, 30))])
    # identical descriptors in one window: the lowest row wins (the rows keep their order: done(shuffle=False)).  The octaves
    # differ between neighbours in that order, or the ratio rule would turn the tie down.
    X = b.back_project(0, 500.0, 420.0, 5.0)
    p = b.point(X, level=1)
    u, v = b.pixel(0, X)
    same = b.near(p, 17)
    tag["identical"] = (p, [b.kp(0, u + dx, v, o, same) for dx, o in ((5.0, 1), (-5.0, 0), (2.0, 1))])
    # over every border, with keypoints outside the image: x = -3 is a candidate of u = 1
    tag["over"] = []
    for (u0, v0), (kx, ky) in (((1.0, 240.0), (-3.0, 240.0)), ((639.0, 200.0), (645.5, 200.0)), ((200.0, 1.0), (200.0, -8.0)),
                               ((260.0, 479.0), (260.0, 485.0)), ((638.0, 478.0), (649.0, 489.0)), ((2.0, 2.0), (-9.0, -9.0))):
        X = b.back_project(0, u0, v0, 5.0)
        p = b.point(X)
        tag["over"].append((p, b.kp(0, kx, ky, 0, b.near(p, 8))))
    # coordinates that are not in the image or not numbers, at octaves that any level 0 window admits
    for x, y in ((NAN, 100.0), (100.0, NAN), (NAN, NAN), (INF, 100.0), (-INF, 100.0), (100.0, INF), (100.0, -INF), (1e30, 1e30),
                 (-1e30, 50.0), (640.0, 100.0), (100.0, 480.0), (-0.0, -0.0), (3e9, -3e9)):
        b.kp(0, x, y, 0)
    # octaves outside 0 .. n_levels - 1 at a level 0 point: -1 is admitted (level - 1), the others are not
    X = b.back_project(0, 80.0, 400.0, 5.0)
    p = b.point(X)
    u, v = b.pixel(0, X)
    tag["octaves"] = (p, [b.kp(0, u + 1.0 + k, v, o, b.near(p, 5 + k)) for k, o in enumerate((-1, -2, 8, 40, I32_MIN, I32_MAX))])
    # frame 2 (count -7) would see all of it
    for i in range(20):
        b.kp(2, 100.0 + 20 * i, 140.0, 7)
    return b.done(tag=tag)


def _random_poses(rng, n):
    poses = np.zeros((n, 7))
    q = np.concatenate([rng.normal(scale=0.05, size=(n, 3)), np.ones((n, 1))], axis=1)
    poses[:, :4] = q / np.linalg.norm(q, axis=1, keepdims=True)
    poses[:, 4:] = rng.uniform(-0.4, 0.4, size=(n, 3))
    return poses


def soup(name="soup", seed=43, n_frames=8, cap=128, n_points=120, params=None):
    """Seeded noise: rotated cameras; points with every status, selection, view count, range and normal; per (frame, point) maybe
    a keypoint near the projection at a likely octave with a near descriptor, maybe a rival, maybe MAPPED or CLAIMED (the point
    is then HELD), maybe claimed without being an inlier; out-of-range ids in the map and the claims; clutter; counts that are 0,
    negative and above cap; a frame that is not searched; twins (two points with one position and one descriptor) that propose
    the same node at the same distance."""
    rng = np.random.default_rng(seed)
    b = _Build(name, n_frames, cap, seed, params=params, poses=_random_poses(rng, n_frames))
    nl = b.prm["n_levels"]
    b.frame_search[0] = 0
    for k in range(n_points):
        f = int(rng.integers(0, n_frames))
        X = b.back_project(f, float(rng.uniform(-60, 700)), float(rng.uniform(-60, 540)), float(rng.uniform(3, 8)) * (-1 if k % 17 == 5 else 1))
        cos = float(rng.choice([1.0, 0.9995, 0.99, 0.9, 0.6, 0.3]))
        scale = float(rng.choice([0.99, 0.99, 0.99, 1.4, 0.7, 3.0, 0.3]))
        b.point(X, f_ref=f, level=int(rng.integers(0, nl)), cos=cos, views=int(rng.choice([1, 2, 5, 0])) if k % 9 == 0 else 3,
                status=int(k % 13 == 4) * 2, select=int(k % 11 != 7), max_scale=scale)
        if k % 10 == 3:  # a twin: the same place, the same descriptor, the next id
            b.points.append(b.points[-1])
    P = len(b.points)
    bad_ids = [-1, -2, -3, -4, P, P + 1, I32_MAX, I32_MIN]
    tag = dict(twins=[p for p in range(1, P) if b.points[p] is b.points[p - 1]])
    for f in range(n_frames):
        room = cap - 24
        for p in rng.permutation(P):
            if len(b.rows[f]) >= room:
                break
            X, _, _, _, _, nrm, (lo, hi) = b.points[p]
            if p in tag["twins"] or rng.random() < 0.45:
                continue
            d, _, uv = sr.project(list(b.poses[f]), X, *INTRINSICS)
            if uv is None:
                continue
            dd = float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
            level = sum(1 for l in range(nl - 1) if b.pw[l] * dd < hi)
            octave = level - int(rng.integers(0, 2)) if rng.random() < 0.85 else int(rng.integers(-2, nl + 2))
            flips = int(rng.integers(0, 45)) if rng.random() < 0.85 else int(rng.integers(90, 130))
            kind = rng.random()
            mapped = dict(node_point=int(p)) if kind < 0.10 else dict(row_point=int(p), row_inlier=1) if kind < 0.16 else \
                dict(row_point=int(p), row_inlier=0) if kind < 0.22 else dict(node_point=int(rng.choice(bad_ids)), row_point=int(rng.choice(bad_ids)), row_inlier=1) if kind < 0.30 else {}
            b.kp(f, uv[0] + float(rng.uniform(-3, 3)), uv[1] + float(rng.uniform(-3, 3)), octave, b.near(p, flips), **mapped)
            if rng.random() < 0.25:
                b.kp(f, uv[0] + float(rng.uniform(-2, 2)), uv[1] + float(rng.uniform(-2, 2)), octave - int(rng.integers(0, 2)),
                     b.near(p, min(flips + int(rng.integers(0, 12)), 200)))
        for _ in range(20):
            x, y = float(rng.uniform(-40, 680)), float(rng.uniform(-40, 520))
            if rng.random() < 0.2:
                x = float(rng.choice([NAN, INF, -INF, -5.0, 640.0, 1e20]))
            b.kp(f, x, y, int(rng.integers(-1, nl + 1)))
    assert n_frames >= 6
    b.counts = {1: 0, 2: -1, 3: cap + 9, 4: len(b.rows[4]) // 2}  # (frame 3: the rows past those laid down exist, and look TAKEN)
    return b.done(shuffle=True, tag=tag)


@functools.lru_cache(maxsize=None)
def soups():
    return (soup(), soup("soup_levels_1", 44, 6, 64, 60, dict(n_levels=1, scale_factor=1.0)),
            soup("soup_levels_32", 45, 6, 64, 60, dict(n_levels=32, scale_factor=1.1)),
            soup("soup_wide", 46, 6, 256, 200, dict(radius_scale=5.0, nn_ratio=0.95, max_hamming=256)),
            soup("soup_small", 47, 6, 32, 40, dict(min_view_cos=-1.0, range_lo=0.0, range_hi=INF)))


def cases():
    return [edges(), windows()] + list(soups())


VARIANTS = ((True, True, True, True), (False, True, True, True), (True, False, True, True), (True, True, False, False),
            (False, False, False, False))  # the map, the claims, status, select


def as_lists(c, use_map=True, use_claims=True, use_status=True, use_select=True):
    """The arguments of search_projection_restate.search."""
    F, cap, P = c["n_frames"], c["cap"], c["n_points"]
    flat = c["desc"].reshape(F * cap, 32)
    fx, fy, cx, cy = c["intrinsics"]
    return dict(kps_x=[float(v) for v in c["kps"][..., 0].reshape(-1)], kps_y=[float(v) for v in c["kps"][..., 1].reshape(-1)],
                kps_octave=c["kps"][..., 5].copy().view(np.int32).reshape(-1).tolist(),
                desc=[int.from_bytes(flat[n].tobytes(), "little") for n in range(F * cap)], counts=c["counts"].tolist(), n_frames=F,
                cap=cap, poses=c["poses"].tolist(), frame_search=c["frame_search"].tolist(),
                node_point_in=c["node_point"].tolist() if use_map else None, row_point_in=c["row_point"].tolist() if use_claims else None,
                row_inlier_in=c["row_inlier"].tolist() if use_claims else None, n_points=P, xyz=c["xyz"].tolist(),
                status=c["status"].tolist() if use_status else None, select=c["select"].tolist() if use_select else None,
                views=c["views"].tolist(), point_desc=[int.from_bytes(c["point_desc"][p].tobytes(), "little") for p in range(P)],
                normal=c["normal"].tolist(), dist=c["dist"].tolist(), fx=fx, fy=fy, cx=cx, cy=cy, width=c["size"][0],
                height=c["size"][1], params=c["params"])


_restated = {}


def restate(c, use_map=True, use_claims=True, use_status=True, use_select=True, rule=None):
    """search_projection_restate.search on the case (computed once per case, variant and rule; do not change the result)."""
    key = (c["name"], id(c["xyz"]), use_map, use_claims, use_status, use_select, rule)
    if key not in _restated:
        _restated[key] = (c, sr.search(rule=rule, **as_lists(c, use_map, use_claims, use_status, use_select)))
    return _restated[key][1]


def as_arrays(e, n_frames):
    """The restated outputs as host arrays."""
    return dict(row_point=np.array(e["row_point"], np.int32), row_inlier=np.array(e["row_inlier"], np.uint8),
                row_dist=np.array(e["row_dist"], np.uint16), frame_totals=np.array(e["frame_totals"], np.int32).reshape(n_frames, 10),
                totals=np.array(e["totals"], np.int32))
