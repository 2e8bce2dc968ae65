"""The undistortion oracle (oracle/undist_oracle.c) on the adversarial classes of tests/undist_cases.py.

Census first: each class is held, with the plain numpy restatement of tests/undist_restate.py and not with the code under
test, to what it was built to reach: table entries at source pixel 0, in the first column and with remapX = -0.0, at which
the five write rules write three different pixel sets (and flipping any one rule changes bytes); clamped indices and the
in-bounds wrap of the last column; pixels whose byte a fused sum would change; tables with no valid entry; outputs around
the 256-thread block.  Then parity: the oracle equals the restatement on every class and mode, byte for byte and in its
`written` mask; it equals the reference's own Undistorter live through oracle/_ref on pinhole pairs that reach the same
places exactly, and the reference's recorded tables and outputs in tests/golden/undist_adversarial.npz
(tools/gen_golden.py undist_adversarial).  The table builder of tests/undist_cases.py is itself pinned there: it reproduces
the reference's tables bit for bit."""
import os

import numpy as np
import pytest

import oracle_lib
import undist_cases as uc
import undist_restate as ur

GOLD = os.path.join(os.path.dirname(__file__), "golden", "undist_adversarial.npz")
MAX_LEFT_OUT = 0.10  # share of pixels the reference leaves undefined, per pair and mode
needs_ref = pytest.mark.skipif(not oracle_lib.have_reference(), reason="oracle/_ref not built")
TABLE_KEYS = ("remapX", "remapFast", "remapIdx", "remapCoef")


def _runs(name):
    """(label, channels, fast, image) of a class"""
    for label, imgs in uc.case(name)["images"]:
        for ch, fast in uc.MODES:
            yield label, ch, fast, imgs[ch]


# ------------------------------------------------------------------------------------------------------------- census
@pytest.mark.parametrize("name", list(uc.CASES))
def test_census(name):
    c = uc.case(name)
    t = c["tables"]
    n_in, n_out = t["w_in"] * t["h_in"], t["w_out"] * t["h_out"]
    x, f, idx, coef = t["remapX"], t["remapFast"], t["remapIdx"], t["remapCoef"]
    assert x.dtype == coef.dtype == np.float32 and f.dtype == idx.dtype == np.int32 and len(x) == n_out
    assert t["w_in"] <= 24 and t["h_in"] <= 16
    for _, imgs in c["images"]:
        assert all(imgs[ch].reshape(-1)[:ch].all() for ch in (1, 3, 4))  # source pixel 0 is non-zero
    # what the plan accepts, and the fast table consistent with remapX
    assert (f < n_in).all() and (idx >= 0).all() and (idx <= n_in + t["w_in"]).all() and not ((f < 0) & (x > 0)).any()
    if name == "origin":
        assert ((x == 0) & ~np.signbit(x) & (f == 0)).any() and ((x == 0) & (f > 0)).any() and (np.signbit(x) & (x == 0)).any()
        assert ((x > 0) & (f == 0)).any() and (x < 0).any()
        masks = {m: ur.write_mask(t, *m) for m in uc.MODES}
        assert np.array_equal(masks[1, True], f > 0) and np.array_equal(masks[3, True], f >= 0)
        assert np.array_equal(masks[4, True], x > 0) and np.array_equal(masks[1, False], ~(x < 0)) and np.array_equal(masks[3, False], x > 0)
        # three different sets: remapFast > 0; remapFast >= 0, which is also !(remapX < 0); remapX > 0 (two rules)
        assert len({m.tobytes() for m in masks.values()}) == 3 and np.array_equal(masks[3, True], masks[1, False])
        assert masks[1, True].sum() < masks[3, True].sum() and masks[4, True].sum() < masks[1, False].sum()
        imgs = c["images"][0][1]
        for wrong, ch, fast in (("fast1_ge", 1, True), ("fast3_gt", 3, True), ("fast4_ge", 4, True), ("bil1_gt", 1, False), ("bil3_ge", 3, False)):
            assert not np.array_equal(ur.undistort(imgs[ch], t, fast)[0], ur.undistort(imgs[ch], t, fast, wrong=wrong)[0]), wrong
    if name == "last_row_col":
        ok = x >= 0
        clamped = (idx >= n_in).any(axis=1)
        wrap = ok & (idx[:, 1] % t["w_in"] == 0) & (idx[:, 1] < n_in)
        assert clamped.sum() >= 8 and wrap.sum() >= 6 and idx.max() == n_in + t["w_in"]
        assert (clamped & (coef[:, 2:] != 0).any(axis=1)).any()  # a clamped source pixel with weight
        img = c["images"][0][1][1]
        assert img.reshape(-1)[n_in - 1] != img.reshape(-1)[n_in - 2]
    if name == "fractions":
        ok = x >= 0
        fx = x - np.trunc(x)
        fr = [np.float32(v) for v in uc.FRACTIONS]
        assert all((fx[ok] == v).any() for v in fr) and all((coef[ok, 3] == np.float32(a) * np.float32(b)).any() for a in fr for b in fr)
        assert [label for label, _ in c["images"]] == ["white", "checker", "random"]
        changed = 0
        for label, ch, fast, img in _runs(name):
            if not fast:
                changed += int((ur.undistort(img, t, False)[0] != ur.undistort(img, t, False, fused=True)[0]).sum())
        assert changed > 0  # a fused sum changes bytes here
    if name == "all_bad":
        assert (x == -1).all() and (f == -1).all() and not idx.any() and not coef.any()
        for label, ch, fast, img in _runs(name):
            assert not ur.undistort(img, t, fast)[0].any()
    if name.startswith("tiny"):
        assert (t["w_out"], t["h_out"], t["w_in"], t["h_in"]) == uc.TINY[name]
        assert n_out in (1, 255, 256, 257, 513)
        assert n_out == 1 or ((x < 0).any() and (x > 0).any())


# ------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(uc.CASES))
def test_oracle_equals_restatement(oracle, name):
    t = uc.case(name)["tables"]
    for label, ch, fast, img in _runs(name):
        want, defined = ur.undistort(img, t, fast)
        got, written = oracle.undistort(img, t, fast=fast)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (name, label, ch, fast, int((got != want).sum()))
        assert np.array_equal(written, defined), (name, label, ch, fast)


def _compare_with_reference(oracle, name, t, imgs, ref_out):
    """the oracle on (t, imgs) against the reference's outputs wherever the reference defines the pixel -> shares left out"""
    shares = {}
    for ch, fast in uc.MODES:
        got, written = oracle.undistort(imgs[ch], t, fast=fast)
        exp = ref_out(ch, fast)
        assert np.array_equal(got[written], exp[written]), (name, ch, fast)
        shares[ch, fast] = 1.0 - written.mean()
        assert shares[ch, fast] <= MAX_LEFT_OUT, (name, ch, fast, shares[ch, fast])
    return shares


def _builder_equals(t, ref_t, name):
    for k in TABLE_KEYS:
        assert np.asarray(t[k]).reshape(-1).tobytes() == np.asarray(ref_t[k]).reshape(-1).tobytes(), (name, k)


@needs_ref
@pytest.mark.parametrize("name", list(uc.REF_PAIRS))
def test_oracle_equals_reference_live(oracle, name):
    cam_in, cam_out = uc.REF_PAIRS[name]
    ru = oracle_lib.RefUndistorter(oracle_lib.load_reference(), cam_in, cam_out)
    try:
        t = ru.tables()
        _builder_equals(uc.ref_tables(name), t, name)
        imgs = uc.ref_images(name)
        shares = _compare_with_reference(oracle, name, t, imgs, lambda ch, fast: ru.run(imgs[ch], fast=fast))
    finally:
        ru.close()
    print(f"reference pair {name}: {t['w_out'] * t['h_out']} pixels, left out per (channels, fast): "
          + ", ".join(f"{m}: {s:.4f}" for m, s in shares.items()))


@pytest.mark.parametrize("name", list(uc.REF_PAIRS))
def test_oracle_equals_recorded_reference(oracle, name):
    g = np.load(GOLD)
    t = {k: g[f"{name}/{k}"] for k in TABLE_KEYS}
    cam_in, cam_out = uc.REF_PAIRS[name]
    t.update(w_in=cam_in[0], h_in=cam_in[1], w_out=cam_out[0], h_out=cam_out[1])
    _builder_equals(uc.ref_tables(name), t, name)
    imgs = {ch: g[f"{name}/img{ch}"] for ch in (1, 3, 4)}
    assert all(np.array_equal(imgs[ch], uc.ref_images(name)[ch]) for ch in imgs)
    _compare_with_reference(oracle, name, t, imgs, lambda ch, fast: g[f"{name}/out{ch}_{int(fast)}"])
    for ch, fast in uc.MODES:  # the recorded masks are the oracle's
        assert np.array_equal(oracle.undistort(imgs[ch], t, fast=fast)[1], g[f"{name}/written{ch}_{int(fast)}"].astype(bool))


def test_reference_pairs_reach_the_edges():
    """what the pinhole pairs reach through the reference's own table code"""
    t = uc.ref_tables("origin")
    x, f = t["remapX"], t["remapFast"]
    assert ((x == 0) & (f == 0)).sum() == 1 and ((x == 0) & (f > 0)).sum() == t["h_out"] - 1 and (x >= 0).all()
    n_in = t["w_in"] * t["h_in"]
    # the last column wraps into the next row; only its last pixel steps past the image
    assert (t["remapIdx"] >= n_in).any(axis=1).sum() == 1 and (t["remapIdx"][:, 1] % t["w_in"] == 0).sum() == t["h_out"]
    t = uc.ref_tables("last_row_col")
    # the whole last row clamps, and the last column's pixel of the row above it
    assert (t["remapIdx"] >= n_in).any(axis=1).sum() == t["w_out"] + 1 and t["remapIdx"].max() == n_in + t["w_in"]
    t = uc.ref_tables("fractions")
    assert (t["remapCoef"] == np.float32(0.25)).all()
