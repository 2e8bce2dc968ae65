"""Adversarial GPU parity of the ORB-SLAM extraction mode: gh_orb_plan_set_distribution(plan, 1) (per-cell FAST +
DistributeOctTree, gslam_amd/csrc/orb_quadtree.hip) and gh_orb_plan_set_steering(plan, 1) (fastAtan2 angle, per-keypoint
pattern rotation, gslam_amd/csrc/orb.hip), alone and together, against oracle.orb_extract in the matching mode -- the
counts, all 28 bytes of every record, all 32 descriptor bytes and the zero tail.

The mode has no debug counters and its three cell kernels launch under one name, so which branch a case reaches is stated
by the host mirrors of tests/orb_slam_mirror.py and asserted next to the case: the cell kernel of every level
(plane32 / plane40 / image), the node table of the tree kernel (512 by the default rule, 1024, 2048), a plan whose key
lists are cut but hold the frame, and one whose list overflows (an error of the call).  tests/test_orb_slam_mode_oracle.py
shows on the CPU that the tie and angle images below do produce the events they are meant to.
"""
import os
import struct
import subprocess

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

import oracle_lib
import orb_slam_mirror as M
from ba_parity import THREADS
from orb_images import CLASSES, TIE_K, TIE_SIZES, symmetric_motifs, tie_images

pytestmark = pytest.mark.gpu

NAMES = sorted(CLASSES)
MODES = [(1, 0), (1, 1), (0, 1)]  # (distribution, steering)
MODE_IDS = ["quadtree", "quadtree+steer", "steer"]


def steer_pattern(reach=(19, 4), seed=3):
    """A test pattern for continuous steering whose farthest points, `reach` and its three quarter-turns, lie at radius
    sqrt(377) = 19.42: inside the accepted 19.49 (x^2 + y^2 <= 379).  The rest is random within that disc."""
    rng = np.random.default_rng(seed)
    pts = rng.integers(-19, 20, (4096, 2))
    pts = pts[(pts ** 2).sum(1) <= 379]
    pat = np.concatenate([pts[:256], pts[256:512]], axis=1).astype(np.int8)
    a, b = reach
    pat[0], pat[1] = (a, b, -a, -b), (-b, a, b, -a)
    pat[2], pat[3] = (b, -a, 0, 0), (-a, -b, 1, 1)
    for t in np.nonzero((pat[:, 0] == pat[:, 2]) & (pat[:, 1] == pat[:, 3]))[0]:
        pat[t, 2:] = (1, 0) if not pat[t, :2].any() else -pat[t, :2]
    assert (pat.astype(np.int32).reshape(-1, 2) ** 2).sum(1).max() == a * a + b * b
    assert not ((pat[:, 0] == pat[:, 2]) & (pat[:, 1] == pat[:, 3])).any()
    return pat


def _plan(ctx, w, h, batch, K, dist=1, steer=0, nlevels=8, ini_th=20, min_th=7, pattern=None):
    from gslam_amd.orb import OrbExtractor
    ex = OrbExtractor(ctx, w, h, max_batch=batch, n_features=K, n_levels=nlevels, ini_th=ini_th, min_th=min_th)
    try:
        ex.set_steering(steer)
        if pattern is not None:
            ex.set_pattern(pattern)
        ex.set_distribution(dist)
    except Exception:
        ex.close()
        raise
    return ex


def _extract(ex, frames, pad=0):
    """One gh_orb_extract_dev call on `frames` laid out with row stride w + pad (pad bytes hold noise that no result may
    depend on) -> (kps B x K x 28 u8, desc B x K x 32, counts)."""
    import torch
    B, h, w = frames.shape
    buf = np.random.default_rng(B * w + pad + 1).integers(0, 256, (B, h, w + pad), dtype=np.uint8)
    buf[:, :, :w] = frames
    kps, desc, counts = ex.extract(torch.from_numpy(buf).cuda())
    torch.cuda.synchronize()
    return (np.ascontiguousarray(kps.cpu().numpy()).view(np.uint8).reshape(B, ex.K, 28), desc.cpu().numpy(),
            counts.cpu().numpy())


def _oracle(oracle, frames, K, dist=1, steer=0, nlevels=8, ini_th=20, min_th=7, pattern=None):
    oracle.orb_set_distribution(dist)
    oracle.orb_set_steer(steer)
    try:
        if pattern is not None:
            assert oracle.orb_set_pattern(pattern)
        ek, ed, ec = oracle.orb_extract_batch(frames, K, nlevels=nlevels, ini_th=ini_th, min_th=min_th, threads=THREADS)
    finally:
        oracle.orb_set_pattern(None)
        oracle.orb_set_distribution(0)
        oracle.orb_set_steer(0)
    return ek.view(np.uint8).reshape(len(ec), K, 28), ed, ec


def _same(got, exp, what):
    """Counts, all 28 + 32 bytes of every live record, and a zero tail; names the first differing frame / record."""
    gk, gd, gc = got
    ek, ed, ec = exp
    B, K = gk.shape[:2]
    bad = np.nonzero(gc != ec)[0]
    assert len(bad) == 0, f"{what}: frame {bad[0]}: count {gc[bad[0]]} vs {ec[bad[0]]} ({len(bad)} frames differ)"
    live = np.arange(K)[None, :] < gc[:, None]
    tail = ~live & ((gk != 0).any(-1) | (gd != 0).any(-1))
    if tail.any():
        f, i = np.argwhere(tail)[0]
        raise AssertionError(f"{what}: frame {f}: record {i} past the count {gc[f]} is not zero")
    diff = live & ((gk != ek).any(-1) | (gd != ed).any(-1))
    if diff.any():
        f, i = np.argwhere(diff)[0]
        raise AssertionError(f"{what}: frame {f} of {B}: record {i} of {gc[f]} differs ({int(diff.sum())} records); "
                             f"keypoint bytes {np.nonzero(gk[f, i] != ek[f, i])[0].tolist()}, descriptor bytes "
                             f"{np.nonzero(gd[f, i] != ed[f, i])[0].tolist()}; got {gk[f, i].view(np.float32)[:5]}, "
                             f"expected {ek[f, i].view(np.float32)[:5]}")


def _case(ctx, oracle, frames, K, pad=0, **mode):
    B, h, w = frames.shape
    ex = _plan(ctx, w, h, B, K, **mode)
    try:
        got = _extract(ex, frames, pad)
    finally:
        ex.close()
    exp = _oracle(oracle, frames, K, **mode)
    _same(got, exp, f"{B} x {w}x{h} (stride {w + pad}) K={K} {mode}")
    return got


def _kernels(oracle, w, h, K, nlevels=8):
    return [M.cell_kernel(oracle, *lv) for lv in M.levels(oracle, w, h, K, nlevels)]


# ---------------------------------------------------------------- 1. every image class in both mode pairs
@pytest.mark.parametrize("w,h,pad", [(160, 120, 3), (100, 77, 12)], ids=["160x120-stride163", "100x77-stride112"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_every_class_in_both_mode_pairs(ctx, oracle, w, h, pad, mode):
    """Both pyramids reach all three cell kernels (level 0 of 100x77 takes slam_cells_kernel straight from the caller's
    16-byte aligned, padded rows; 160x120's stride 163 is staged).  One plan per mode, two distinct frames per class."""
    dist, steer = mode
    K = 600
    ks = _kernels(oracle, w, h, K)
    assert {"plane32", "plane40", "image"} <= set(ks), ks
    if w == 100:
        assert ks[0] == "image" and (w + pad) % 16 == 0
    ex = _plan(ctx, w, h, 2, K, dist, steer)
    try:
        for c, name in enumerate(NAMES):
            frames = np.stack([CLASSES[name](w, h, 17 * c + 5 * f) for f in range(2)])
            got = _extract(ex, frames, pad)
            _same(got, _oracle(oracle, frames, K, dist, steer), f"{name} {w}x{h} {mode}")
    finally:
        ex.close()


# ---------------------------------------------------------------- 2. ties that decide the tree
@pytest.mark.parametrize("w,h", TIE_SIZES)
def test_tie_lattices(ctx, oracle, w, h):
    """Checkerboards of period 2 .. 6 and dot lattices: many nodes hold equal key counts (stage (B) order by y0, x0) and
    equal responses (the per-node maximum and the final cut decide by y, x); stage (B) repeats on several of them."""
    assert max(oracle.orb_quotas(TIE_K[0])) <= 3 and max(oracle.orb_quotas(TIE_K[1])) <= 3
    imgs = tie_images(w, h)
    frames = np.stack(list(imgs.values()))
    for K in TIE_K:
        for steer in ((0, 1) if K == 300 else (0,)):
            ex = _plan(ctx, w, h, len(frames), K, 1, steer)
            try:
                got = _extract(ex, frames, 5)
            finally:
                ex.close()
            _same(got, _oracle(oracle, frames, K, 1, steer), f"tie lattices {w}x{h} K={K} steer={steer} ({list(imgs)})")


# ---------------------------------------------------------------- 3. angle edges of continuous steering
@pytest.mark.parametrize("mode", [(1, 1), (0, 1)], ids=["quadtree+steer", "steer"])
@pytest.mark.parametrize("custom", [False, True], ids=["builtin-pattern", "radius-19.42-pattern"])
def test_angle_edges(ctx, oracle, mode, custom):
    """Point-symmetric patches (m10 = m01 = 0), patches mirror-symmetric about either axis (angle exactly 0, 90, 180, 270)
    and about either diagonal, with the built-in pattern and with one that reaches radius 19.42."""
    w, h, K = 320, 240, 800
    frames = np.stack([symmetric_motifs(w, h, ["point"]), CLASSES["sym_axes"](w, h, 0), CLASSES["sym_axes"](w, h, 3),
                       CLASSES["sym_point"](w, h, 5)])
    pat = steer_pattern() if custom else None
    ex = _plan(ctx, w, h, len(frames), K, *mode, pattern=pat)
    try:
        got = _extract(ex, frames, 7)
    finally:
        ex.close()
    exp = _oracle(oracle, frames, K, *mode, pattern=pat)
    _same(got, exp, f"angle edges {mode} custom={custom}")
    live = np.arange(K)[None, :] < got[2][:, None]
    ang = set(got[0][live][:, 12:16].copy().view(np.float32).ravel().tolist())
    assert {0.0, 90.0, 180.0, 270.0, oracle.orb_fast_atan2_deg(1.0, 1.0), oracle.orb_fast_atan2_deg(1.0, -1.0)} <= ang


def test_pattern_radius_limit(ctx, oracle):
    """A point at radius sqrt(377) is accepted for continuous steering and refused by the 30-bin table; radius sqrt(386) =
    19.65 (the next sum of two squares above 379) is refused by both, on the plan and by the oracle."""
    from gslam_amd import hip
    ok, bad = steer_pattern((19, 4)), steer_pattern((19, 5))
    ex = _plan(ctx, 160, 120, 1, 300)
    try:
        with pytest.raises(hip.GslamHipError):
            ex.set_pattern(ok)
        ex.set_steering(1)
        ex.set_pattern(ok)
        with pytest.raises(hip.GslamHipError):
            ex.set_pattern(bad)
    finally:
        ex.close()
    oracle.orb_set_steer(1)
    try:
        assert oracle.orb_set_pattern(ok) and not oracle.orb_set_pattern(bad)
    finally:
        oracle.orb_set_pattern(None)
        oracle.orb_set_steer(0)


# ---------------------------------------------------------------- 4. geometry edges
GEOMETRY = [  # w, h, K, nlevels, ini_th, min_th, what the case is for
    (4096, 50, 1000, 8, 20, 7, "226 / 338 roots, level-0 x up to 4076 in the 12-bit key field"),
    (4096, 40, 1000, 8, 20, 7, "508 roots: 2032 table entries"),
    (60, 1500, 600, 8, 20, 7, "portrait strip: one root, a deep tree"),
    (333, 257, 9416, 8, 20, 7, "level-0 quota 2045: the 2048 table full"),
    (72, 300, 300, 8, 20, 7, "level 0 one column of 40-px cells: plane40"),
    (73, 300, 300, 8, 20, 7, "level 0 one column of 41-px cells: image"),
    (91, 120, 300, 8, 20, 7, "59-px cells: image at its widest"),
    (113, 97, 300, 8, 20, 7, "two columns of 41-px cells: image"),
    (64, 64, 100, 8, 20, 7, "32-px cells: plane32 at its widest"),
    (333, 257, 700, 1, 30, 5, "one level"),
    (333, 257, 700, 2, 254, 1, "two levels, no strong cells"),
    (333, 257, 1500, 8, 9, 8, "ini_th = min_th + 1"),
]


@pytest.mark.parametrize("i", range(len(GEOMETRY)), ids=[f"{g[0]}x{g[1]}-K{g[2]}-L{g[3]}" for g in GEOMETRY])
def test_geometry_edges(ctx, oracle, i):
    w, h, K, nl, ini, mn, what = GEOMETRY[i]
    assert not M.refused(oracle, w, h, K, nl), what
    ks = _kernels(oracle, w, h, K, nl)
    expect0 = {72: "plane40", 73: "image", 91: "image", 113: "image", 64: "plane32"}.get(w)
    if expect0:
        assert ks[0] == expect0, (what, ks)
    if w == 4096:
        roots = [M.n_roots(lw, lh) for lw, lh, q in M.levels(oracle, w, h, K, nl) if M.live(lw, lh, q)]
        assert roots == ([226, 338] if h == 50 else [508]), roots
        assert M.tree_nodes(oracle, w, h, K, nl, 2) == 2048
    if K == 9416:
        assert oracle.orb_quotas(K)[0] == 2045 and M.tree_nodes(oracle, w, h, K, nl, 2) == 2048
    frames = np.stack([CLASSES["noise"](w, h, i), CLASSES["sym_axes" if i % 2 else "dots5"](w, h, i)])
    kps, _, counts = _case(ctx, oracle, frames, K, pad=1 + i, dist=1, steer=i % 2, nlevels=nl, ini_th=ini, min_th=mn)
    assert counts[0] > 0
    if w == 4096 and h == 50:  # keypoints near the right end of level 0 came through the 12-bit x of the key
        x = kps[0, :counts[0]].copy().view(np.float32).reshape(-1, 7)[:, 0]
        assert x.max() >= 4000


@pytest.mark.parametrize("w,h,K", [(4096, 39, 1000), (333, 257, 9420)], ids=["4096x39-2324-roots", "quota-2046"])
def test_geometry_refused(ctx, oracle, w, h, K):
    """One step past each limit: 4 * 581 roots > 2048, and a level-0 quota of 2046 (+ 3 > 2048): the mode is refused."""
    from gslam_amd import hip
    from gslam_amd.orb import OrbExtractor
    assert M.refused(oracle, w, h, K)
    if K == 9420:
        assert oracle.orb_quotas(K)[0] == 2046
    ex = OrbExtractor(ctx, w, h, max_batch=1, n_features=K)
    try:
        with pytest.raises(hip.GslamHipError):
            ex.set_distribution(1)
    finally:
        ex.close()


# ---------------------------------------------------------------- 5. tree capacity by the default rule
@pytest.mark.parametrize("nodes,w,h,K,B", [(512, 96, 80, 500, 256), (1024, 96, 80, 3000, 256), (2048, 333, 257, 6000, 2)])
def test_tree_capacity_by_default_rule(ctx, oracle, nodes, w, h, K, B):
    """No override: 256 frames x 8 levels (2048 workgroups) with quotas <= 509 take the 512-entry table; the same launch with
    a quota of 652 must not (1024); a quota of 1303 takes 2048."""
    assert "GSLAM_HIP_QT_NODES" not in os.environ
    assert M.tree_nodes(oracle, w, h, K, 8, B) == nodes
    frames = np.stack([CLASSES[NAMES[f % len(NAMES)]](w, h, 31 + f) for f in range(B)])
    _case(ctx, oracle, frames, K, pad=2, dist=1, steer=int(nodes == 1024))


# ---------------------------------------------------------------- 6. the overflow contract
def test_key_budget_overflow_is_an_error_of_the_call(ctx, oracle):
    """Two plans one max_batch apart around the point where the key budget stops holding a noise frame's candidates
    (mirrored caps, exact candidate counts of the oracle): the first is cut but holds them (oracle bytes), the second
    overflows (GslamHipError) and then serves a frame that fits (oracle bytes: the flag was cleared)."""
    from gslam_amd import hip
    w, h, K, nl = 640, 480, 1000, 1
    noise = np.stack([CLASSES["noise"](w, h, 11 + i) for i in range(2)])
    fits = CLASSES["mixed"](w, h, 4)[None]
    cnt = np.max([M.candidate_counts(oracle, f, K, nl) for f in noise], axis=0)

    def over(B):
        caps, _ = M.key_caps(oracle, w, h, K, nl, B)
        return any(c > cp for c, cp in zip(cnt, caps))

    lo, hi = 1, 65535
    assert over(hi)
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if over(mid) else (mid + 1, hi)
    b_over = lo
    caps_fit, cut_fit = M.key_caps(oracle, w, h, K, nl, b_over - 1)
    caps_over, _ = M.key_caps(oracle, w, h, K, nl, b_over)
    assert cut_fit and all(c <= cp for c, cp in zip(cnt, caps_fit)), (cnt, caps_fit)
    assert all(c <= cp for c, cp in zip(M.candidate_counts(oracle, fits[0], K, nl), caps_over))
    exp = _oracle(oracle, noise, K, nlevels=nl)
    ex = _plan(ctx, w, h, b_over - 1, K, nlevels=nl)
    try:
        assert ex.device_bytes() <= 32 << 30, ex.device_bytes()
        _same(_extract(ex, noise), exp, f"cut plan (max_batch {b_over - 1}, caps {caps_fit}, candidates {cnt.tolist()})")
    finally:
        ex.close()
    ex = _plan(ctx, w, h, b_over, K, nlevels=nl)
    try:
        assert ex.device_bytes() <= 32 << 30, ex.device_bytes()
        with pytest.raises(hip.GslamHipError, match="overflowed"):
            _extract(ex, noise)
        _same(_extract(ex, fits), _oracle(oracle, fits, K, nlevels=nl), f"overflowed plan (max_batch {b_over}), next call")
    finally:
        ex.close()


# ---------------------------------------------------------------- 7. fuzz
@settings(max_examples=40, deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture, HealthCheck.data_too_large])
@given(w=st.integers(39, 260), h=st.integers(39, 200), pad=st.sampled_from([0, 1, 3, 16, 61]),
       K=st.one_of(st.integers(1, 40), st.integers(41, 3000)), nlevels=st.integers(1, 8),
       min_th=st.one_of(st.integers(1, 12), st.integers(13, 254)), ini_extra=st.one_of(st.just(0), st.integers(1, 60)),
       name=st.sampled_from(NAMES), seed=st.integers(0, 2 ** 31 - 1), batch=st.integers(1, 3), steer=st.booleans())
def test_fuzz_slam_mode(ctx, oracle, w, h, pad, K, nlevels, min_th, ini_extra, name, seed, batch, steer):
    ini_th = min(254, min_th + ini_extra)
    if M.refused(oracle, w, h, K, nlevels):  # (one level of quota > 2045)
        from gslam_amd import hip
        with pytest.raises(hip.GslamHipError):
            _plan(ctx, w, h, batch, K, 1, int(steer), nlevels, ini_th, min_th).close()
        return
    frames = np.stack([CLASSES[name](w, h, seed + i) for i in range(batch)])
    _case(ctx, oracle, frames, K, pad=pad, dist=1, steer=int(steer), nlevels=nlevels, ini_th=ini_th, min_th=min_th)


# ---------------------------------------------------------------- 8. stream and plugin
def test_stream_bgr_in_slam_mode(ctx, oracle):
    """gh_orb_stream_* with BGR input, both modes set on the stream's plan: fixed-point luma on the device, then steps 4',
    5', 6', 8' -- against oracle.bgr_to_gray + orb_extract."""
    from gslam_amd import hip
    from gslam_amd.orb import OrbStream
    w, h, K = 333, 257, 700
    st_ = OrbStream(ctx, w, h, 3, 2, channels=3, n_features=K)
    try:
        plan = hip.lib.gh_orb_stream_plan(st_.s)
        ctx.check(hip.lib.gh_orb_plan_set_steering(plan, 1))
        ctx.check(hip.lib.gh_orb_plan_set_distribution(plan, 1))
        rng = np.random.default_rng(9)
        imgs = []
        for c, name in enumerate(["sym_axes", "checker3", "noise"]):
            g = CLASSES[name](w, h, c)
            im = np.stack([g, g, g], -1).astype(np.int32)
            im += rng.integers(-6, 7, im.shape)
            imgs.append(np.clip(im, 0, 255).astype(np.uint8))
        off, kps, desc, _ = st_.collect(st_.submit(np.ascontiguousarray(np.stack(imgs)).reshape(3, -1)))
    finally:
        st_.close()
    oracle.orb_set_distribution(1)
    oracle.orb_set_steer(1)
    try:
        exp = [oracle.orb_extract(oracle.bgr_to_gray(im), K) for im in imgs]
    finally:
        oracle.orb_set_distribution(0)
        oracle.orb_set_steer(0)
    for f, (ek, ed) in enumerate(exp):
        assert off[f + 1] - off[f] == len(ek) > 0, f
        assert kps[off[f]:off[f + 1]].tobytes() == ek.tobytes(), f"frame {f}: keypoints differ"
        assert np.array_equal(desc[off[f]:off[f + 1]], ed), f"frame {f}: descriptors differ"


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "oracle", "_ref", "bin", "plugin_host")
LIBDIR = os.path.join(ROOT, "gslam_amd", "lib")
PLUGDIR = os.path.join(ROOT, "oracle", "_ref", "plugins")


@pytest.mark.parametrize("name", ["sym_axes", "checker4", "dots5", "noise"])
def test_slam_mode_through_featuredetector_plugin(tmp_path, oracle, name):
    if not (os.path.exists(HOST) and os.path.exists(os.path.join(PLUGDIR, "libgslam_featuredetector.so"))):
        pytest.skip("oracle/_ref/bin/plugin_host or libgslam_featuredetector.so missing (run `make plugins` where the GSLAM headers are)")
    w, h, K = 640, 480, 1500
    img = CLASSES[name](w, h, 21)
    inp, out = tmp_path / "img.raw", tmp_path / "out.bin"
    img.tofile(inp)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIBDIR + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    env["GSLAM_HOST_SVAR"] = "FeatureDetectorHIP.Steering=1;FeatureDetectorHIP.Distribution=1"
    r = subprocess.run([HOST, "orb", PLUGDIR, str(w), str(h), "1", str(inp), str(out), str(K)], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    oracle.orb_set_distribution(1)
    oracle.orb_set_steer(1)
    try:
        ek, ed = oracle.orb_extract(img, K)
    finally:
        oracle.orb_set_distribution(0)
        oracle.orb_set_steer(0)
    raw = open(out, "rb").read()
    ok, n, _, _ = struct.unpack("4i", raw[:16])
    assert ok == 1 and n == len(ek) > 0, r.stdout + r.stderr
    assert np.frombuffer(raw, oracle_lib.KP_DTYPE, n, 16).tobytes() == ek.tobytes()
    assert np.array_equal(np.frombuffer(raw, np.uint8, n * 32, 16 + n * 28).reshape(n, 32), ed)
