"""CPU proof of the quantised pass 1 of orb_fast_cells (gslam_amd/csrc/orb.hip: fast_compass4_q), in numpy uint32.

Phase A above ini_th filters with a compass test on pixels quantised to 6 bits, q(x) = x >> 2, four pixels per dword in 8-bit
fields with bit 7 as the guard: with t' = (T + 1) >> 2, A = q(c) + t' + 127 and D = q(c) - t' + 128 per field,
  bit 7 of A - q(x)  <=>  q(x) <= q(c) + t' - 1   (x is certainly not brighter than c + T)
  bit 7 of D - q(x)  <=>  q(x) <= q(c) - t'       (x is possibly darker than c - T)
and no field borrows from its neighbour.  Pass 2 scores every queued pixel exactly, so the filter only has to pass a SUPERSET
of the exact compass test, which passes a superset of {S > T}.  Both are shown here: the field arithmetic exhaustively, the
superset on the oracle's pyramid levels and score maps.  No GPU.
"""
import numpy as np
import pytest

from orb_phase_b_cases import compass

K4 = np.uint32(0x01010101)
KQ = np.uint32(0x3F3F3F3F)
GUARD = np.uint32(0x80808080)


def quant4(w):
    """q of the four bytes of every dword: (w >> 2) & 0x3F3F3F3F"""
    return (w >> np.uint32(2)) & KQ


def consts(T):
    """CompassQ of orb.hip -> (a, d): t' + 127 and 128 - t' in every byte"""
    tq = (int(T) + 1) >> 2
    return np.uint32(((tq + 127) * 0x01010101) & 0xFFFFFFFF), np.uint32(((128 - tq) * 0x01010101) & 0xFFFFFFFF)


def alignbyte(hi, lo, n):
    """v_alignbyte_b32: the low dword of {hi, lo} >> 8 n, n = 1 .. 3"""
    return (lo >> np.uint32(8 * n)) | (hi << np.uint32(32 - 8 * n))


def compass4_q(T, wc, wl, wr, wu, wd):
    """fast_compass4_q, instruction by instruction -> flags of pixels 0 .. 3 at bits 7, 15, 23, 31 (the rest masked off)"""
    ka, kd = consts(T)
    c, u, d = quant4(wc), quant4(wu), quant4(wd)
    l, r = quant4(alignbyte(wc, wl, 1)), quant4(alignbyte(wr, wc, 3))
    A, D = c + ka, c + kd
    bright = ~((A - u) & (A - d)) & ~((A - l) & (A - r))
    dark = ((D - u) | (D - d)) & ((D - l) | (D - r))
    return (bright | dark) & GUARD


def compass_q(img, T):
    """The quantised pass 1 on a whole image, dword by dword as the kernel reads its tile (aligned dwords, the dwords left,
    right, three rows up and down) -> bool map, False where compass() of tests/orb_phase_b_cases.py is not defined"""
    h, w = img.shape
    nd = (w + 3) // 4
    P = np.zeros((h + 6, 4 * (nd + 2)), np.uint8)
    P[3:3 + h, 4:4 + w] = img
    dw = P.view("<u4")
    flags = compass4_q(T, dw[3:-3, 1:-1], dw[3:-3, :-2], dw[3:-3, 2:], dw[:-6, 1:-1], dw[6:, 1:-1])
    px = np.stack([(flags >> np.uint32(8 * k + 7)) & np.uint32(1) for k in range(4)], axis=-1).reshape(h, 4 * nd)[:, :w].astype(bool)
    out = np.zeros((h, w), bool)
    out[3:-3, 3:-3] = px[3:-3, 3:-3]
    return out


@pytest.fixture(scope="module")
def pairs():
    c, x = np.meshgrid(np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32), indexing="ij")
    return c.ravel(), x.ravel()


def test_field_arithmetic_is_exhaustively_the_stated_predicate(pairs):
    """all c, x in 0 .. 255 and all T in 0 .. 255, alone in field 0: bit 7 of A - q(x) and of D - q(x) are the two predicates,
    and the field never leaves 1 .. 255 (so nothing reaches bit 8)"""
    c, x = pairs
    qc, qx = (c >> np.uint32(2)).astype(np.int64), (x >> np.uint32(2)).astype(np.int64)
    for T in range(256):
        tq = (T + 1) >> 2
        ka, kd = consts(T)
        A = quant4(c) + (ka & np.uint32(0xFF))
        D = quant4(c) + (kd & np.uint32(0xFF))
        a, d = A - quant4(x), D - quant4(x)
        assert a.min() >= 1 and a.max() <= 255 and d.min() >= 1 and d.max() <= 255, (T, a.min(), a.max(), d.min(), d.max())
        assert np.array_equal((a >> np.uint32(7)) & np.uint32(1), (qx <= qc + tq - 1).astype(np.uint32)), T
        assert np.array_equal((d >> np.uint32(7)) & np.uint32(1), (qx <= qc - tq).astype(np.uint32)), T


@pytest.mark.parametrize("field", range(4))
def test_fields_do_not_borrow_from_each_other(pairs, field):
    """the pair (c, x) in one field, 0 and 255 as centre and neighbour in the three other fields (all four combinations): bit 7
    of every other field is what that field gives alone, bit 7 of this one what it gives alone, for every T"""
    c, x = pairs
    sh = np.uint32(8 * field)
    others = np.uint32(0xFFFFFFFF) ^ (np.uint32(0xFF) << sh)
    for T in range(256):
        ka, kd = consts(T)
        for k in (ka, kd):
            alone = ((quant4(c << sh) + (k & ~others)) - quant4(x << sh)) & GUARD
            for cn in (0, 255):
                for xn in (0, 255):
                    wc = (c << sh) | (np.uint32(cn * 0x01010101) & others)
                    wx = (x << sh) | (np.uint32(xn * 0x01010101) & others)
                    got = ((quant4(wc) + k) - quant4(wx)) & GUARD
                    solo = (np.uint32((cn >> 2) * 0x01010101) + k - np.uint32((xn >> 2) * 0x01010101)) & GUARD & others
                    assert np.array_equal(got & ~others, alone), (T, cn, xn)
                    assert (got & others == solo).all(), (T, cn, xn)


def test_implications_hold_for_every_byte_triple():
    """x >= c + T + 1 implies q(x) >= q(c) + t' and x <= c - T - 1 implies q(x) <= q(c) - t': the quantised flags can only be a
    superset of the exact ones"""
    c, x = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for T in range(256):
        tq = (T + 1) >> 2
        br, dk = x >= c + T + 1, x <= c - T - 1
        assert ((x[br] >> 2) >= (c[br] >> 2) + tq).all() and ((x[dk] >> 2) <= (c[dk] >> 2) - tq).all(), T


THRESHOLDS = (1, 2, 3, 20, 21, 22, 23, 45, 51, 254, 255)


@pytest.fixture(scope="module")
def levels(oracle):
    out = []
    for f in range(3):
        img = oracle.synth_frame(640, 480, 0x5EED0000 + f)
        for l in (0, 2, 5):
            lvl = img if l == 0 else oracle.orb_pyramid_level(img, l)
            out.append((f, l, lvl, oracle.orb_score_map(lvl, 1).astype(np.int32)))
    return out


@pytest.mark.parametrize("T", THRESHOLDS)
def test_quantised_survivors_contain_the_exact_ones_on_score_maps(levels, T):
    """levels 0, 2, 5 of three synthetic 640x480 frames: {S > T} within the exact compass set within the quantised one.  The
    survivor ratio (what pass 2 pays) is printed, not asserted."""
    ratios = []
    for f, l, lvl, S in levels:
        exact, quant = compass(lvl, T), compass_q(lvl, T)
        scored = S > T
        assert not (scored & ~exact).any(), (f, l, T, np.argwhere(scored & ~exact)[:3].tolist())
        assert not (exact & ~quant).any(), (f, l, T, np.argwhere(exact & ~quant)[:3].tolist())
        if exact.sum():
            ratios.append(quant.sum() / exact.sum())
        print(f"T={T} frame {f} level {l}: scored {int(scored.sum())} exact {int(exact.sum())} quantised {int(quant.sum())}")
    if ratios:
        print(f"T={T}: quantised / exact survivors {min(ratios):.3f} .. {max(ratios):.3f}")
