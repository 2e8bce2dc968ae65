"""CPU census and the rules of the threshold hint of large ORB calls (gslam_amd/csrc/orb.hip: fast_cells_tile, select_weak_cells,
hint_next), restated in Python on the oracle's own pyramid and score map.

The rule: phase A of the two-phase detector may run a (level, frame) at any threshold T with ini_th <= T <= 255.  A cell's
record then holds its candidates above T with their true ranks.  If at least quota[l] cells hold such a candidate (T-strong
cells), the level's output is what the complete records give; otherwise the whole level has to be redone.  The plan keeps one
T per (level, batch slot), which orb_select derives from the score at the quota cut of each call, and a hold-off that keeps a
slot at ini_th after it had to be redone.  tests/test_orb_threshold_hint_cpu.py proves the rule,
tests/test_orb_threshold_hint_gpu.py holds the kernels to it.
"""
import functools

import numpy as np

from orb_phase_b_cases import CELL, EDGE, INI_TH, MIN_TH

HINT_MAX_HOLD = 64
HINT_NUM, HINT_DEN = 2, 3  # T goes this fraction of the way from ini_th to the cut score


def level_cells(oracle, lvl, min_th=MIN_TH):
    """One pyramid level -> dict: S (the oracle's score map), cand (strict 3 x 3 maxima of S), ncx, ncy; None without cells."""
    h, w = lvl.shape
    vw, vh = w - 2 * EDGE, h - 2 * EDGE
    if vw <= 0 or vh <= 0:
        return None
    S = oracle.orb_score_map(lvl, min_th)
    Si = S.astype(np.int32)
    P = np.pad(Si, 1)
    nb = np.max([P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)], axis=0)
    return {"S": S, "cand": (Si > 0) & (Si > nb), "ncx": (vw + CELL - 1) // CELL, "ncy": (vh + CELL - 1) // CELL}


def frame_cells(oracle, img, nlevels=8, min_th=MIN_TH):
    img = np.ascontiguousarray(img)
    return [level_cells(oracle, img if l == 0 else oracle.orb_pyramid_level(img, l, nlevels), min_th) for l in range(nlevels)]


def _cell_max(c, mask):
    """[ncy, ncx]: the largest score among the pixels of `mask` in every cell (0: none)"""
    h, w = c["S"].shape
    p = np.zeros((c["ncy"] * CELL, c["ncx"] * CELL), np.int32)
    v = np.where(mask, c["S"].astype(np.int32), 0)[EDGE:h - EDGE, EDGE:w - EDGE]
    p[:v.shape[0], :v.shape[1]] = v
    return p.reshape(c["ncy"], CELL, c["ncx"], CELL).max(axis=(1, 3))


def t_strong_cells(c, T):
    """cells that hold a candidate above T"""
    return int((_cell_max(c, c["cand"]) > T).sum())


def premise(c, quota, T):
    return quota > 0 and t_strong_cells(c, T) >= quota


def cut_at(c, T):
    """The score map that phase A at T leaves: everything at or below T zeroed."""
    return np.where(c["S"] > T, c["S"], 0).astype(np.uint8)


def cut_score(c, quota, ini_th=INI_TH):
    """The score s* of entry number `quota` of the level's order (oracle step 5) if that entry has rank 0, else None.  A cell's
    rank-0 entry is its best candidate, and every rank-0 entry comes before every other: s* is the quota-th best of the cells'
    best candidates, where that many cells hold one."""
    top = _cell_max(c, c["cand"])
    tops = np.sort(top[top > 0])[::-1]
    return int(tops[quota - 1]) if len(tops) >= quota else None


def hint_from_cut(s, ini_th=INI_TH):
    return ini_th + (s - ini_th) * HINT_NUM // HINT_DEN if s is not None and s > ini_th else ini_th


HINT_FIRST_EPOCH = 256


def hint_threshold(state, epoch, ini_th=INI_TH):
    """what the adaptive call number `epoch` of a plan runs a (level, slot) at: a slot with a penalty goes above ini_th in calls
    of even epoch only, so that the call in between learns of the mispredictions of the whole plan before the next attempt"""
    t, _, pen = state
    return ini_th if pen > 0 and epoch % 2 == 1 else t


def hint_next(state, s, mispredicted, others=False, ini_th=INI_TH, t_used=None):
    """state = (T, hold, penalty) of one (level, slot) -> its state after a call whose quota cut was s (cut_score) and that ran
    at t_used (hint_threshold; default: T).
    mispredicted: this (level, slot) was redone; others: some (level, slot) of the previous call was.  A slot that is not
    holding takes that for its own, with a hold one call shorter (it learns of it one call late); one that is holding keeps
    at least that hold: the holds of a plan end together"""
    t, hold, pen = state
    t = t if t_used is None else t_used
    if mispredicted or (others and hold == 0):
        pen = 2 if pen == 0 else min(2 * pen, HINT_MAX_HOLD)
        return ini_th, pen if mispredicted else pen - 1, pen
    if hold > 0:
        return ini_th, max(hold - 1, pen - 1) if others else hold - 1, pen
    if t > ini_th and pen > 0:
        pen -= 1
    return hint_from_cut(s, ini_th), 0, pen


class HintModel:
    """The plan's advice for `batch` slots, driven by the CPU census of each call's frames."""

    def __init__(self, batch, quotas, ini_th=INI_TH):
        self.quotas, self.ini_th = quotas, ini_th
        self.state = [[(ini_th, 0, 0)] * 8 for _ in range(batch)]
        self.mispredicted = []  # (call, slot, level)
        self.calls = 0
        self.epoch = HINT_FIRST_EPOCH
        self.last_call_mispredicted = False  # the plan-wide signal: some (level, slot) of the previous call was redone

    def call(self, census):
        """census[slot][level] = level_cells(...) of the frame in that slot"""
        self.epoch += 1
        for b, levels in enumerate(census):
            for l, c in enumerate(levels):
                q = self.quotas[l]
                if c is None or q <= 0:
                    continue
                t = hint_threshold(self.state[b][l], self.epoch, self.ini_th)
                mis = t > self.ini_th and t_strong_cells(c, t) < q
                if mis:
                    self.mispredicted.append((self.calls, b, l))
                others = self.last_call_mispredicted
                self.state[b][l] = hint_next(self.state[b][l], cut_score(c, q, self.ini_th), mis, others, self.ini_th, t)
        self.last_call_mispredicted = any(c == self.calls for c, _, _ in self.mispredicted)
        self.calls += 1

    def hints(self):
        return np.array([[s[0] for s in row] for row in self.state], np.uint8)


@functools.lru_cache(maxsize=None)
def textured_frames(oracle, n, w=640, h=480):
    fr = np.stack([oracle.synth_frame(w, h, 0x5EED0000 + f) for f in range(n)])
    fr.setflags(write=False)
    return fr
