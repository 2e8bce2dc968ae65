"""CPU evidence for the inputs of tests/test_orb_slam_mode_gpu.py: the ORB-SLAM mode has no debug counters, so what the GPU
cases are meant to reach is shown here on the oracle and on the independent Python restatement of the quadtree
(tests/test_orb_oracle.py::_quadtree_py) -- tie events of the tree on the tie lattices, exact special angles of continuous
steering on the symmetric motifs -- and the host mirrors of tests/orb_slam_mirror.py are held to the numbers the issue of
the mode states."""
import numpy as np
import pytest

import orb_slam_mirror as M
from orb_images import CLASSES, TIE_K, TIE_SIZES, tie_images
from test_orb_oracle import _quadtree_py

UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]  # GH_ORB_UMAX: the radius-15 disc


def _moments(img, x, y):
    m10 = m01 = 0
    for v in range(-15, 16):
        u = np.arange(-UMAX[abs(v)], UMAX[abs(v)] + 1)
        row = img[y + v, x + u].astype(np.int64)
        m10 += int((u * row).sum())
        m01 += v * int(row.sum())
    return m10, m01


@pytest.mark.parametrize("w,h", TIE_SIZES)
def test_tie_lattices_make_the_tie_rules_decide(oracle, w, h):
    """On the GPU case's images and K: the restatement equals the oracle level by level, and every tie rule of step 5'
    decides somewhere -- stage (B) runs (and repeats), orders nodes of equal key count, nodes hold several maxima of equal S,
    the cut to N (quotas of 1 .. 3 included) passes over an equal S."""
    total = {}
    repeats = small_cuts = 0
    for name, img in tie_images(w, h).items():
        for l, (lw, lh, _) in enumerate(M.levels(oracle, w, h, 1000)):
            if not M.live(lw, lh, 1):
                continue
            lvl = img if l == 0 else oracle.orb_pyramid_level(img, l)
            cx, cy, cs = oracle.orb_slam_candidates(oracle.orb_score_map(lvl, 7), 20)
            if len(cx) == 0:
                continue
            cands = list(zip(cx.tolist(), cy.tolist(), cs.tolist()))
            for N in sorted({int(oracle.orb_quotas(K)[l]) for K in TIE_K} - {0}):
                st = {}
                ox, oy, os_ = oracle.orb_quadtree(cx, cy, cs, lw, lh, N)
                assert list(zip(ox.tolist(), oy.tolist(), os_.tolist())) == _quadtree_py(cands, lw, lh, N, st), (name, l, N)
                repeats += st["b_passes"] > 1
                small_cuts += N <= 3 and st["cuts"] > 0 and st["cut_ties"] > 0
                for k, v in st.items():
                    total[k] = total.get(k, 0) + v
    assert total["b_passes"] > 0 and total["b_equal_counts"] > 0 and total["node_max_ties"] > 0, total
    assert total["cuts"] > 0 and total["cut_ties"] > 0, total
    assert repeats > 0 and small_cuts > 0, (repeats, small_cuts)


@pytest.mark.parametrize("dist", [1, 0])
def test_symmetric_motifs_hit_the_special_angles(oracle, dist):
    """The angle images of the GPU case give level-0 keypoints whose moments are exactly (0, 0), (+-m, 0), (0, +-m) and
    (m, m) / (-m, m), and whose continuous angles are exactly 0, 180, 90, 270 and fastAtan2's 44.99 / 135.01; the sin / cos
    quadrant k = (int)(a / 90 + 0.5) then leaves a remainder of exactly 0 on the axes."""
    w, h, K = 320, 240, 800
    seen = {}
    for img in (CLASSES["sym_point"](w, h, 5), CLASSES["sym_axes"](w, h, 0), CLASSES["sym_axes"](w, h, 3)):
        oracle.orb_set_distribution(dist)
        oracle.orb_set_steer(1)
        try:
            kps, _ = oracle.orb_extract(img, K)
        finally:
            oracle.orb_set_distribution(0)
            oracle.orb_set_steer(0)
        for k in kps[kps["octave"] == 0]:
            m10, m01 = _moments(img, int(k["x"]), int(k["y"]))
            assert k["angle"] == np.float32(oracle.orb_fast_atan2_deg(float(m01), float(m10)))
            key = ("zero" if m10 == 0 and m01 == 0 else "x+" if m01 == 0 and m10 > 0 else "x-" if m01 == 0 else
                   "y+" if m10 == 0 and m01 > 0 else "y-" if m10 == 0 else "diag" if m10 == m01 else
                   "anti" if m10 == -m01 else "other")
            seen.setdefault(key, set()).add(float(k["angle"]))
    d, a = oracle.orb_fast_atan2_deg(1.0, 1.0), oracle.orb_fast_atan2_deg(1.0, -1.0)
    assert d != 45.0 and a != 135.0  # (so no angle lands on a tie of the quadrant rounding)
    want = {"zero": {0.0}, "x+": {0.0}, "x-": {180.0}, "y+": {90.0}, "y-": {270.0}, "diag": {d}, "anti": {a}}
    for key, angles in want.items():
        assert seen.get(key) == angles, (key, seen.get(key))
    for ang, k in ((0.0, 0), (90.0, 1), (180.0, 2), (270.0, 3)):
        assert int(np.float32(ang) / np.float32(90.0) + np.float32(0.5)) == k
        cs, sn = oracle.orb_sincos_deg(ang)
        assert (cs, sn) == ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[k]


def test_mirrors_agree_with_the_stated_limits(oracle):
    """The host mirrors against the numbers of gh_qt_create / gh_qt_tree: cell kernel classes by level width, the 4096 x 40 /
    x 39 root limit, the quota-2045 limit, the 512 table by the default rule, and where the key budget starts cutting."""
    cls = {lw: M.cell_kernel(oracle, lw, 64, 1) for lw in (39, 64, 65, 72, 73, 91, 92, 96, 97, 112, 113, 121, 122)}
    assert cls == {39: "plane32", 64: "plane32", 65: "plane40", 72: "plane40", 73: "image", 91: "image", 92: "plane32",
                   96: "plane32", 97: "plane40", 112: "plane40", 113: "image", 121: "image", 122: "plane32"}, cls
    assert M.cell_kernel(oracle, 38, 300, 1) is None and M.cell_kernel(oracle, 300, 300, 0) is None
    assert not M.refused(oracle, 4096, 40, 1000) and M.refused(oracle, 4096, 39, 1000)
    assert M.n_roots(4096, 40) == 508 and M.n_roots(4096, 39) == 581 and M.n_roots(150, 420) == 1
    k2045 = min(K for K in range(9000, 9500) if oracle.orb_quotas(K)[0] == 2045)
    k2046 = min(K for K in range(9000, 9500) if oracle.orb_quotas(K)[0] == 2046)
    assert not M.refused(oracle, 333, 257, k2045) and M.refused(oracle, 333, 257, k2046)
    assert (k2045, k2046) == (9416, 9420) or oracle.orb_quotas(9416)[0] == 2045 and oracle.orb_quotas(9420)[0] == 2046
    assert M.tree_nodes(oracle, 96, 80, 500, 8, 256) == 512 and M.tree_nodes(oracle, 96, 80, 500, 8, 255) == 1024
    assert M.tree_nodes(oracle, 96, 80, 3000, 8, 256) == 1024 and M.tree_nodes(oracle, 333, 257, 6000, 8, 1) == 2048
    for (w, h), first_cut in (((1920, 1080), 441), ((640, 480), 3378)):
        assert not M.key_caps(oracle, w, h, 1000, 8, first_cut - 1)[1] and M.key_caps(oracle, w, h, 1000, 8, first_cut + 1)[1]
