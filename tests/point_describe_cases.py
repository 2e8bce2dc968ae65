"""Inputs for gh_describe_points_dev, shared by tests/test_point_describe_cpu.py (what they reach) and
tests/test_point_describe_gpu.py (the device against tests/point_describe_restate.py).  A case is a dict of host arrays: kps
(n_frames x cap x 7 float32 view of the KeyPoint records: the octave is written as int32 bits into column 5), desc (n_frames x
cap x 32 uint8), counts, poses (n_frames x 7), obs_cam / obs_point / obs_node (n_obs int32), obs_use (n_obs uint8), n_points,
xyz, status (int32), select (uint8) and the three parameters.  A track may put several nodes into one frame: the stage does
not care, and it keeps the arrays small."""
import functools

import numpy as np

import point_describe_restate as pr

OUTPUTS = ("point_state", "point_desc", "point_obs", "point_views", "point_normal", "point_dist", "totals")
DTYPE = dict(point_state=np.uint8, point_desc=np.uint8, point_obs=np.int32, point_views=np.int32, point_normal=np.float64,
             point_dist=np.float64, totals=np.int32)
WIDTH = dict(point_state=1, point_desc=32, point_obs=2, point_views=1, point_normal=3, point_dist=2)  # entries per point
SOUP_LENGTHS = (1, 2, 3, 7, 8, 9, 16, 17, 63, 64, 65, 127, 128, 200)  # both sides of 8 and of 64, and the stride formula
SOUP_MAX_VIEWS = (64, 1, 5, 8, 9)
OCTAVES = (-3, 0, 7, 40, 1, 2, 3, 4, 5, 6)  # the first four on the references of the first tracks: both ends of the clamp
MAX_FLIPS = 59
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def _flip(rng, base, k):
    """`base` (32 bytes) with k distinct bits flipped."""
    d = base.copy()
    for bit in rng.choice(256, size=k, replace=False):
        d[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return d


def _make(name, lengths, n_frames, cap, seed, max_views=64, scale_factor=1.2, n_levels=8, identical=False, shuffle=True,
          n_empty=3, masked_extra=True, not_ok=(), skipped=(), counts=None):
    """Tracks of the given lengths (after the dropped observations are taken out) on distinct nodes, the point ids permuted, the
    observation list shuffled; not_ok / skipped: indices into `lengths` of tracks whose point is marked so."""
    rng = np.random.default_rng(seed)
    if counts is None:
        counts = rng.integers(cap - 5, cap + 1, size=n_frames).astype(np.int32)
        counts[-1] = cap + 7  # clamped to cap
    rows = np.clip(counts, 0, cap)
    nodes = np.concatenate([f * cap + np.arange(rows[f]) for f in range(n_frames)])
    nodes = rng.permutation(nodes)
    n_tracks = len(lengths)
    n_points = n_tracks + n_empty
    ids = rng.permutation(n_points)[:n_tracks]
    kps = np.zeros((n_frames, cap, 7), np.float32)
    kps[..., :2] = rng.uniform(0, 600, size=(n_frames, cap, 2)).astype(np.float32)
    octave = rng.choice(OCTAVES, size=n_frames * cap).astype(np.int32)
    desc = rng.integers(0, 256, size=(n_frames * cap, 32), dtype=np.uint8)
    poses = np.zeros((n_frames, 7))
    q = rng.normal(size=(n_frames, 4))
    poses[:, :4] = q / np.linalg.norm(q, axis=1, keepdims=True)
    poses[:, 4:] = rng.uniform(-2, 2, size=(n_frames, 3))
    xyz = rng.uniform(-1, 1, size=(n_points, 3)) + np.array([0.0, 0.0, 6.0])
    obs_point, obs_node, obs_use = [], [], []
    at = 0
    for t, L in enumerate(lengths):
        mine = nodes[at:at + L]
        assert len(mine) == L, "not enough nodes"
        at += L
        base = rng.integers(0, 256, size=32, dtype=np.uint8)
        for n in mine:
            desc[n] = base if identical else _flip(rng, base, int(rng.integers(0, MAX_FLIPS + 1)))
        obs_point += [int(ids[t])] * L
        obs_node += [int(n) for n in mine]
        obs_use += [1] * L
        if masked_extra and t % 3 == 0 and at < len(nodes):  # a masked observation on a node of its own: L must not count it
            obs_point.append(int(ids[t]))
            obs_node.append(int(nodes[at]))
            obs_use.append(0)
            at += 1
    order = rng.permutation(len(obs_point)) if shuffle else np.arange(len(obs_point))
    obs_point = np.array(obs_point, np.int32)[order]
    obs_node = np.array(obs_node, np.int32)[order]
    obs_use = np.array(obs_use, np.uint8)[order]
    # the references of the first tracks see the four octaves of the clamp
    for t in range(min(n_tracks, 8)):
        ks = np.flatnonzero((obs_point == ids[t]) & (obs_use != 0))
        if len(ks):
            octave[obs_node[ks[0]]] = OCTAVES[t % 4]
    kps[..., 5] = octave.reshape(n_frames, cap).view(np.float32)
    status = np.zeros(n_points, np.int32)
    select = np.ones(n_points, np.uint8)
    for t in not_ok:
        status[ids[t]] = 1 + t % 5  # every GH_TRACK_* that is not OK
    for t in skipped:
        select[ids[t]] = 0
    return dict(name=name, n_frames=n_frames, cap=cap, kps=kps, desc=desc.reshape(n_frames, cap, 32), counts=counts, poses=poses,
                obs_cam=(obs_node // cap).astype(np.int32), obs_point=obs_point, obs_node=obs_node, obs_use=obs_use, n_points=n_points,
                xyz=xyz, status=status, select=select, max_views=max_views, scale_factor=scale_factor, n_levels=n_levels,
                track_ids=ids, lengths=tuple(lengths))


@functools.lru_cache(maxsize=None)
def soup(max_views=64):
    """Every length of SOUP_LENGTHS twice; of each length the second copy's point is left as it is, and three more tracks are
    NOT_OK, SKIPPED and both.  The geometry does not depend on max_views."""
    lengths = SOUP_LENGTHS + SOUP_LENGTHS + (5, 12, 70)
    k = len(SOUP_LENGTHS)
    return _make("soup_mv%d" % max_views, lengths, 8, 256, seed=21, max_views=max_views, not_ok=(2 * k, 2 * k + 2),
                 skipped=(2 * k + 1, 2 * k + 2))


@functools.lru_cache(maxsize=None)
def identical():
    """Every observation of a track has the same descriptor: every rule ties, candidate 0 must win."""
    return _make("identical", (1, 2, 3, 8, 9, 64, 65, 100), 4, 128, seed=22, identical=True)


@functools.lru_cache(maxsize=None)
def levels():
    """Other pyramids: the clamp at another bound, one level (min = max = dist), the largest table."""
    return tuple(_make("levels_%d" % n, (1, 2, 3, 4, 5, 9, 11, 20), 4, 64, seed=23 + n, scale_factor=s, n_levels=n)
                 for n, s in ((1, 1.0), (3, 2.0), (32, 1.2), (5, 1.4142135623730951)))


@functools.lru_cache(maxsize=None)
def drops():
    """Every way an observation can be dropped, each planted into tracks that stay valid without it: masked; obs_point and obs_node
    out of range with poisoned values; a node past counts (in a short frame, in a frame whose count is negative, and never in
    the frame whose count exceeds cap: that one is clamped and its last row exists); obs_cam unequal to the node's frame."""
    cap, n_frames = 32, 5
    counts = np.array([32, 20, -3, 39, 31], np.int32)
    c = _make("drops", (2, 3, 4, 5, 9, 10), n_frames, cap, seed=24, counts=counts, masked_extra=True, shuffle=False)
    N = n_frames * cap
    p0, p1, p2 = (int(v) for v in c["track_ids"][:3])
    good_node = int(c["obs_node"][0])
    extra = []  # (cam, point, node, use, why)
    for bad in (-1, c["n_points"], c["n_points"] + 1, I32_MAX, I32_MIN):
        extra.append((good_node // cap, bad, good_node, 1, "point"))
    for bad in (-1, N, N + 1, I32_MAX, I32_MIN, -cap):
        extra.append((0, p0, bad, 1, "node"))
    for node in (1 * cap + 20, 1 * cap + 31, 2 * cap + 0, 2 * cap + 31, 4 * cap + 31):
        extra.append((node // cap, p1, node, 1, "count"))
    for cam in (-1, n_frames, I32_MAX, I32_MIN):
        extra.append((cam, p2, 0 * cap + 3, 1, "cam"))
    extra.append((1, p2, 0 * cap + 3, 1, "cam"))           # another valid frame
    extra.append((3, p0, 3 * cap + 31, 1, "kept"))         # counts[3] = 39 clamps to cap: row 31 exists, the observation counts
    extra.append((0, p1, 0 * cap + 5, 0, "masked"))
    rng = np.random.default_rng(7)
    n_old = len(c["obs_point"])
    cam = np.concatenate([c["obs_cam"], np.array([e[0] for e in extra], np.int32)])
    point = np.concatenate([c["obs_point"], np.array([e[1] for e in extra], np.int32)])
    node = np.concatenate([c["obs_node"], np.array([e[2] for e in extra], np.int32)])
    use = np.concatenate([c["obs_use"], np.array([e[3] for e in extra], np.uint8)])
    order = rng.permutation(len(cam))
    why = np.array([""] * n_old + [e[4] for e in extra])[order]
    return dict(c, obs_cam=cam[order], obs_point=point[order], obs_node=node[order], obs_use=use[order], why=why)


@functools.lru_cache(maxsize=None)
def centre():
    """A point at a camera centre: as the reference (dist = 0 and a NaN direction), as a later observation of a short track, and
    as a late observation of a long one."""
    c = _make("centre", (3, 5, 20, 4), 4, 64, seed=25, masked_extra=False)
    xyz = c["xyz"].copy()
    e = restate(c)
    for t, live in ((0, 0), (1, 3), (2, 17)):
        p = int(c["track_ids"][t])
        k = e["tracks"][p][live]
        xyz[p] = c["poses"][c["obs_node"][k] // c["cap"], 4:]
    return dict(c, xyz=xyz)


@functools.lru_cache(maxsize=None)
def long_track():
    """One track of 4096 observations among 500 short ones."""
    rng = np.random.default_rng(26)
    lengths = tuple(int(v) for v in rng.integers(2, 7, size=500))
    lengths = lengths[:250] + (4096,) + lengths[250:]
    return _make("long", lengths, 16, 512, seed=26, n_empty=11)


def cases():
    return [soup(mv) for mv in SOUP_MAX_VIEWS] + [identical(), drops(), centre(), long_track()] + list(levels())


def as_lists(c, use_obs_use=True, use_status=True, use_select=True):
    """The arguments of point_describe_restate.describe, as lists."""
    F, cap = c["n_frames"], c["cap"]
    octave = c["kps"][..., 5].copy().view(np.int32).reshape(-1).tolist()
    flat = c["desc"].reshape(F * cap, 32)
    desc = [int.from_bytes(flat[n].tobytes(), "little") for n in range(F * cap)]
    return dict(kps_octave=octave, desc=desc, counts=c["counts"].tolist(), n_frames=F, cap=cap, poses=c["poses"].tolist(),
                obs_cam=c["obs_cam"].tolist(), obs_point=c["obs_point"].tolist(), obs_node=c["obs_node"].tolist(),
                obs_use=c["obs_use"].tolist() if use_obs_use else None, n_points=c["n_points"], xyz=c["xyz"].tolist(),
                status=c["status"].tolist() if use_status else None, select=c["select"].tolist() if use_select else None,
                scale_factor=c["scale_factor"], n_levels=c["n_levels"], max_views=c["max_views"])


_restated = {}


def restate(c, use_obs_use=True, use_status=True, use_select=True):
    """point_describe_restate.describe on the case (computed once per case and variant; do not change the result)."""
    key = (c["name"], id(c["xyz"]), use_obs_use, use_status, use_select)
    if key not in _restated:
        _restated[key] = (c, pr.describe(**as_lists(c, use_obs_use, use_status, use_select)))  # (c is kept alive: id() stays its)
    return _restated[key][1]


def as_arrays(e, n_points, before=None):
    """The restated outputs as host arrays.  before: the in/out arrays as they went in (dict of arrays at capacity); the SKIPPED
    points keep those bytes.  None: zeros."""
    out = {}
    state = np.array(e["point_state"], np.uint8).reshape(n_points)
    desc = np.zeros((n_points, 32), np.uint8)
    for p, d in enumerate(e["point_desc"]):
        desc[p] = np.frombuffer(int(d).to_bytes(32, "little"), np.uint8)
    out["point_state"] = state
    out["point_desc"] = desc
    out["point_obs"] = np.array(e["point_obs"], np.int32).reshape(n_points, 2)
    out["point_views"] = np.array(e["point_views"], np.int32).reshape(n_points)
    out["point_normal"] = np.array(e["point_normal"], np.float64).reshape(n_points, 3)
    out["point_dist"] = np.array(e["point_dist"], np.float64).reshape(n_points, 2)
    out["totals"] = np.array(e["totals"], np.int32)
    if before is not None:
        skipped = state == pr.SKIPPED
        for k in WIDTH:
            if k != "point_state":
                out[k][skipped] = before[k].reshape(out[k].shape)[skipped]
    return out
