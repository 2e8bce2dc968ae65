"""Host mirrors of the dispatch rules of the ORB-SLAM extraction mode (gh_orb_plan_set_distribution(plan, 1)), for the
tests that must say which branch of gslam_amd/csrc/orb_quadtree.hip a case reaches.  The mode has no debug counters and its
three cell kernels launch under one name, so these restatements are the only witness; each one names the code it mirrors.
"""
import numpy as np

EDGE = 19            # GH_ORB_EDGE: a level of w <= 38 or h <= 38 gets quota 0 (gh_qt_create)
QT_NODES = 2048      # kQtNodes: quota + 3 and 4 * roots must fit the largest table
CELL_MAX = 59        # kCellMax: wc, hc above it are refused
WC_MAX = 32          # kWcMax: slam_cells_plane_kernel<false>
PC_BIG = 40          # kPcBig: slam_cells_plane_kernel<true> (gh_qt_plane_ok)
KEY_BUDGET = (4 << 30) // 6   # bytes of keys (4) + node ids (2) that a plan may hold over all of its frames
COUNT_BITS = 22      # the count field of stage (B)'s sort key


def levels(oracle, w, h, K, nlevels=8):
    """[(lw, lh, quota)] of every level (gh_orb_plan_create / oracle_orb_level_dims + oracle_orb_quotas)."""
    ws, hs = oracle.orb_level_dims(w, h, nlevels)
    return list(zip(ws.tolist(), hs.tolist(), oracle.orb_quotas(K, nlevels).tolist()))


def live(lw, lh, quota):
    """Whether gh_qt_create keeps the level's quota (w, h > 2 * EDGE and quota > 0)."""
    return lw > 2 * EDGE and lh > 2 * EDGE and quota > 0


def n_roots(lw, lh):
    """nIni = max(1, roundf(W' / H')), fp32 division, round half away from zero."""
    r = float(np.float32(lw - 32) / np.float32(lh - 32))
    return max(1, int(np.floor(r + 0.5)))


def cell_kernel(oracle, lw, lh, quota):
    """Which kernel takes the level's cells (orb.hip enqueue_quadtree + gh_qt_cells): None (quota 0),
    'plane32' (slam_cells_plane_kernel<false>), 'plane40' (<true>) or 'image' (slam_cells_kernel, which reads the level
    itself: a level without a plane but with a quota, i.e. wc or hc > 40)."""
    if not live(lw, lh, quota):
        return None
    _, _, wc, hc = oracle.orb_slam_grid(lw, lh)
    m = max(wc, hc)
    return "plane32" if m <= WC_MAX else "plane40" if m <= PC_BIG else "image"


def refused(oracle, w, h, K, nlevels=8):
    """Whether gh_qt_create refuses the plan (gh_orb_plan_set_distribution(plan, 1) fails)."""
    for lw, lh, q in levels(oracle, w, h, K, nlevels):
        if not live(lw, lh, q):
            continue
        if lw > 4096 or lh > 4096 or q + 3 > QT_NODES:
            return True
        _, _, wc, hc = oracle.orb_slam_grid(lw, lh)
        if 4 * n_roots(lw, lh) > QT_NODES or wc > CELL_MAX or hc > CELL_MAX:
            return True
    return False


def tree_nodes(oracle, w, h, K, nlevels, batch):
    """The node table the tree kernel runs with (gh_qt_create's need, gh_qt_tree's choice): 512 only when every level fits
    it AND the launch has at least 2048 workgroups, else the least of 1024 / 2048 that fits."""
    need = 0
    for lw, lh, q in levels(oracle, w, h, K, nlevels):
        if live(lw, lh, q):
            need = max(need, q + 3, 4 * n_roots(lw, lh))
    least = 512 if need <= 512 else 1024 if need <= 1024 else 2048
    if least <= 512 and nlevels * batch >= 2048:
        return 512
    return 1024 if least <= 1024 else 2048


def worst_keys(oracle, w, h, K, nlevels=8):
    """Per level: the most candidates its cells can hold, ncols nrows ceil(wc / 2) ceil(hc / 2) (0 for a dead level)."""
    out = []
    for lw, lh, q in levels(oracle, w, h, K, nlevels):
        if not live(lw, lh, q):
            out.append(0)
            continue
        nc, nr, wc, hc = oracle.orb_slam_grid(lw, lh)
        out.append(nc * nr * ((wc + 1) // 2) * ((hc + 1) // 2))
    return out


def key_caps(oracle, w, h, K, nlevels, max_batch):
    """(caps, cut): the key slots of every level per frame and whether any is below its worst case (gh_qt_create)."""
    worst = worst_keys(oracle, w, h, K, nlevels)
    total = sum(worst)
    budget = KEY_BUDGET // max_batch
    caps = []
    for wl in worst:
        cap = int(float(wl) * float(budget) / float(total)) if total > budget else wl
        caps.append(min(cap, (1 << COUNT_BITS) - 1))
    return caps, any(c < wl for c, wl in zip(caps, worst))


def candidate_counts(oracle, img, K, nlevels=8, ini_th=20, min_th=7):
    """Exact number of candidates every level of `img` appends to its key list (oracle steps 2 and 4'); 0 on dead levels."""
    h, w = img.shape
    out = []
    for l, (lw, lh, q) in enumerate(levels(oracle, w, h, K, nlevels)):
        if not live(lw, lh, q):
            out.append(0)
            continue
        lvl = img if l == 0 else oracle.orb_pyramid_level(img, l, nlevels)
        cx, _, _ = oracle.orb_slam_candidates(oracle.orb_score_map(lvl, min_th), ini_th)
        out.append(len(cx))
    return out
