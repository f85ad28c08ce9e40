"""GPU parity of the pictures (viz_kernels.hip through vppx_error_colors / vppx_guided_visualize / vppx_colorize _dev and _host,
vppx_finite_max_dev, the Engine methods and the vppstereo_amd.utils drop-in).  Everything is compared byte for byte against
tests/_viz_ref.py -- which tests/test_viz_cpu.py holds to the reference's own output -- and, for dilation <= 1, against that
output itself (tests/golden/viz_cases.npz); the code under test is never the checker.  The shapes are chosen for where the
kernel can break (its tile is 64 x 16 pixels, DESIGN "pictures"), not for the workload; one call runs at 540 x 960."""
import ctypes as C
import os

import numpy as np
import pytest

import _viz_ref as VR
from vppstereo_amd import _lib

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 16
KEYS = VR.KEYS
SENTINEL = 0xA5
# brightest rows of the colour table, one per error: per channel their maximum is (248, 243, 254)
BRIGHT = np.array([2.0, 4.5, 7.0], np.float32)


@pytest.fixture(scope="module")
def eng():
    from vppstereo_amd.engine import Engine
    return Engine()


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "viz_cases.npz"))


def _t(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _special():
    sp = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viz_cases.npz"))["special"]
    return sp


def _data(B, H, W, seed, bleed=False):
    """(disp, gt, valid) whose |disp - gt| walks over all bins, with the golden file's edge values, NaN and +-inf sprinkled in
    and valid drawn from {0, 1, 0.5, -1}.  bleed: the last row of every frame gets the brightest colours, the first row of every
    frame is black."""
    rng = np.random.default_rng(seed)
    n = B * H * W
    err = (rng.uniform(0, 1, n) ** 3 * 70).astype(np.float32)
    gt = rng.uniform(1, 60, n).astype(np.float32)
    sp = _special()
    at = rng.choice(n, size=min(n // 2, 3 * len(sp)), replace=False)
    gt[at] = 0
    err[at] = np.resize(sp, len(at))      # exact: disp - 0
    disp = gt + err * rng.choice(np.array([-1, 1], np.float32), n)
    odd = rng.choice(n, size=max(1, n // 40), replace=False)
    disp[odd[0::4]] = np.nan
    gt[odd[1::4]] = np.nan
    disp[odd[2::4]] = np.inf
    gt[odd[3::4]] = -np.inf
    valid = rng.choice(np.array([0, 1, 0.5, -1], np.float32), n, p=[0.3, 0.4, 0.15, 0.15]).astype(np.float32)
    disp, gt, valid = (a.astype(np.float32).reshape(B, H, W) for a in (disp, gt, valid))
    if bleed:
        gt[:, -1] = 5
        disp[:, -1] = 5 + np.resize(BRIGHT, W)
        valid[:, -1] = 1
        valid[:, 0] = 0
    return disp, gt, valid


def _ref_guided(disp, gt, valid, scale, d):
    """[6, B, H, W, 3]"""
    B = disp.shape[0]
    per = [VR.guided_visualize(disp[f], gt[f], valid[f], scale, d) for f in range(B)]
    return np.stack([np.stack([per[f][k] for f in range(B)]) for k in KEYS])


def _ref_errors(errors, mask, scale, bgr, d):
    return np.stack([VR.error_colors(errors[f], scale, None if mask is None else mask[f], bgr, d) for f in range(errors.shape[0])])


def _err_of(disp, gt):
    with np.errstate(invalid="ignore"):
        return np.abs(disp - gt)


def _guided(eng, disp, gt, valid, scale=1, d=7, which=None):
    import torch
    out = torch.full((6,) + disp.shape + (3,), SENTINEL, dtype=torch.uint8, device=eng.device)
    r = eng.guided_visualize(_t(eng, disp), _t(eng, gt), _t(eng, valid), scale=scale, dilation=d, which=which, out=out)
    return r, _np(out)


def _check_guided(eng, disp, gt, valid, scale, d, tag):
    r, out = _guided(eng, disp, gt, valid, scale, d)
    assert tuple(r) == KEYS
    want = _ref_guided(disp, gt, valid, scale, d)
    for n, k in enumerate(KEYS):
        bad = np.argwhere(out[n] != want[n])
        assert bad.size == 0, (tag, k, len(bad), bad[:4].tolist())
        assert np.array_equal(_np(r[k]), want[n])


# ---------------------------------------------------------------------------------------------------------------------
# pinned to the reference itself (dilation 0 and 1)
# ---------------------------------------------------------------------------------------------------------------------
def test_error_colors_equal_the_reference_output(eng, cases):
    e = cases["ce_errors"][None]
    for scale in (1, 3, 19):
        for bgr in (True, False):
            for dil in (0, 1):
                for mname in ("none", "mask", "mask2"):
                    mask = None if mname == "none" else cases["ce_" + mname][None]
                    got = _np(eng.error_colors(_t(eng, e), None if mask is None else _t(eng, mask), scale=scale, bgr=bgr, dilation=dil))
                    want = cases[f"ce_out_s{scale}_b{int(bgr)}_d{dil}_{mname}"]
                    assert got.dtype == np.uint8 and got.shape == (1,) + want.shape
                    assert np.array_equal(got[0], want), (scale, bgr, dil, mname, np.argwhere(got[0] != want)[:4].tolist())


def test_guided_visualize_equals_the_reference_output(eng, cases):
    d, g, v = (cases[k][None] for k in ("gv_disp", "gv_gt", "gv_valid"))
    for scale in (1, 3, 19):
        for dil in (0, 1):
            _, out = _guided(eng, d, g, v, scale, dil)
            want = cases[f"gv_out_s{scale}_d{dil}"]
            for n, k in enumerate(KEYS):
                assert np.array_equal(out[n, 0], want[n]), (scale, dil, k, np.argwhere(out[n, 0] != want[n])[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# shapes and dilations against the numpy restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [7, 15])
def test_frame_smaller_than_the_window(eng, d):
    disp, gt, valid = _data(1, 3, 5, seed=d)
    valid[0, 1, 2] = 1
    disp[0, 1, 2], gt[0, 1, 2] = 9, 2
    _check_guided(eng, disp, gt, valid, 1, d, f"3x5 d{d}")
    e = _err_of(disp, gt)
    assert np.array_equal(_np(eng.error_colors(_t(eng, e), _t(eng, valid), dilation=d)), _ref_errors(e, valid, 1, True, d))


@pytest.mark.parametrize("d", [0, 1, 2, 3, 4, 7])
def test_odd_sizes_three_frames_no_bleed(eng, d):
    """37 x 67: odd, no multiple of 4, so rows start at every byte alignment; three frames adjacent in memory, the last row
    of each in the brightest colours and the first row of the next black: a window that crosses a frame border shows."""
    disp, gt, valid = _data(3, 37, 67, seed=100 + d, bleed=True)
    _check_guided(eng, disp, gt, valid, 1, d, f"37x67 d{d}")
    want = _ref_guided(disp, gt, valid, 1, d)
    assert (want[4][:, -1].max(axis=1) == (248, 243, 254)).all()      # the bright last rows are in the expected picture
    if d <= 1:
        assert (want[4][:, 0] == 0).all()
    e, m = _err_of(disp, gt), valid
    for bgr in (True, False):
        got = _np(eng.error_colors(_t(eng, e), _t(eng, m), scale=19, bgr=bgr, dilation=d))
        assert np.array_equal(got, _ref_errors(e, m, 19, bgr, d)), (d, bgr)
    got = _np(eng.error_colors(_t(eng, e), None, dilation=d))
    assert np.array_equal(got, _ref_errors(e, None, 1, True, d))


@pytest.mark.parametrize("B,H,W", [(1, TILE_H + 1, TILE_W + 1), (2, TILE_H, TILE_W), (1, 2 * TILE_H + 3, 2 * TILE_W)])
@pytest.mark.parametrize("d", [1, 4, 7])
def test_tile_edges(eng, B, H, W, d):
    disp, gt, valid = _data(B, H, W, seed=H * W + d)
    _check_guided(eng, disp, gt, valid, 3, d, f"{B}x{H}x{W} d{d}")


def test_a_frame_does_not_depend_on_its_batch(eng):
    disp, gt, valid = _data(3, 21, 70, seed=9)
    _, all3 = _guided(eng, disp, gt, valid, 1, 7)
    for f in range(3):
        _, one = _guided(eng, disp[f:f + 1], gt[f:f + 1], valid[f:f + 1], 1, 7)
        assert np.array_equal(one[:, 0], all3[:, f])


@pytest.mark.parametrize("which", [1, 2, 4, 8, 16, 32, 63])
def test_which_writes_only_the_selected_planes(eng, which):
    disp, gt, valid = _data(2, 19, 23, seed=which)
    r, out = _guided(eng, disp, gt, valid, 1, 3, which=which)
    want = _ref_guided(disp, gt, valid, 1, 3)
    assert tuple(r) == tuple(k for n, k in enumerate(KEYS) if which >> n & 1)
    for n, k in enumerate(KEYS):
        if which >> n & 1:
            assert np.array_equal(out[n], want[n]), k
        else:
            assert (out[n] == SENTINEL).all(), k
    if which == 16:
        r2, out2 = _guided(eng, disp, gt, valid, 1, 3, which="avgerr")
        assert tuple(r2) == ("avgerr",) and np.array_equal(out2, out)


def test_maximum_supported_dilation(eng):
    disp, gt, valid = _data(1, 40, 70, seed=31)
    valid[valid == 1] = 0        # sparse picture: a box of 31 would fill a dense one
    _check_guided(eng, disp, gt, valid, 1, _lib.VIZ_MAX_DILATION, "d31")


# ---------------------------------------------------------------------------------------------------------------------
# the four ways in: _dev == _host == Engine == drop-in
# ---------------------------------------------------------------------------------------------------------------------
def test_dev_host_engine_and_dropin_agree(eng):
    import torch
    from vppstereo_amd import utils as U
    lib, h = eng.lib, eng.ctx.handle
    disp, gt, valid = _data(1, 29, 45, seed=77)
    want = _ref_guided(disp, gt, valid, 3, 7)
    # guided_visualize
    _, via_engine = _guided(eng, disp, gt, valid, 3, 7)
    host = np.full((6, 1, 29, 45, 3), SENTINEL, np.uint8)
    _lib.check(lib.vppx_guided_visualize_host(h, 1, 29, 45, _lib.np_ptr(disp), _lib.np_ptr(gt), _lib.np_ptr(valid), 3.0, 7, 63, _lib.np_ptr(host)))
    td, tg, tv = _t(eng, disp), _t(eng, gt), _t(eng, valid)
    dev = torch.full((6, 1, 29, 45, 3), SENTINEL, dtype=torch.uint8, device=eng.device)
    eng._bind_stream()
    _lib.check(lib.vppx_guided_visualize_dev(h, 1, 29, 45, td.data_ptr(), tg.data_ptr(), tv.data_ptr(), 3.0, 7, 63, dev.data_ptr()))
    drop = U.guided_visualize(disp[0], gt[0], valid[0], scale=3)     # the reference's default dilation is 7
    assert tuple(drop) == KEYS
    for n, k in enumerate(KEYS):
        assert np.array_equal(via_engine[n], want[n]) and np.array_equal(host[n], want[n]) and np.array_equal(_np(dev)[n], want[n])
        assert drop[k].shape == (29, 45, 3) and drop[k].dtype == np.uint8 and np.array_equal(drop[k], want[n, 0]), k
    # _host leaves the planes that were not asked for alone
    host2 = np.full((6, 1, 29, 45, 3), SENTINEL, np.uint8)
    _lib.check(lib.vppx_guided_visualize_host(h, 1, 29, 45, _lib.np_ptr(disp), _lib.np_ptr(gt), _lib.np_ptr(valid), 3.0, 7, 32, _lib.np_ptr(host2)))
    assert np.array_equal(host2[5], want[5]) and (host2[:5] == SENTINEL).all()
    # error colours
    e = _err_of(disp, gt)
    want_e = _ref_errors(e, valid, 1, False, 4)
    via_engine = _np(eng.error_colors(_t(eng, e), _t(eng, valid), bgr=False, dilation=4))
    host = np.full((1, 29, 45, 3), SENTINEL, np.uint8)
    _lib.check(lib.vppx_error_colors_host(h, 1, 29, 45, _lib.np_ptr(e), _lib.np_ptr(valid), 1.0, 0, 4, _lib.np_ptr(host)))
    te = _t(eng, e)
    dev = torch.full((1, 29, 45, 3), SENTINEL, dtype=torch.uint8, device=eng.device)
    eng._bind_stream()
    _lib.check(lib.vppx_error_colors_dev(h, 1, 29, 45, te.data_ptr(), tv.data_ptr(), 1.0, 0, 4, dev.data_ptr()))
    drop = U.color_error_image_kitti(e[0], mask=valid[0], BGR=False, dilation=4)
    for got in (via_engine, host, _np(dev), drop[None]):
        assert np.array_equal(got, want_e)
    # a boolean mask, as test.py:327 passes it, and the defaults
    assert np.array_equal(U.color_error_image_kitti(e[0], mask=gt[0] > 0), VR.error_colors(e[0], 1, gt[0] > 0, True, 1))
    assert np.array_equal(U.color_error_image_kitti(e[0]), VR.error_colors(e[0]))


# ---------------------------------------------------------------------------------------------------------------------
# colour-mapped maps and max_val
# ---------------------------------------------------------------------------------------------------------------------
def _cmap_data(seed):
    rng = np.random.default_rng(seed)
    B, H, W = 2, 21, 67
    mv = np.array([37.25, 191.0], np.float32)       # two frames, two ranges
    x = rng.uniform(-5, 220, (B, H, W)).astype(np.float32)
    for f in range(B):
        vals = [0, -0.0, mv[f], np.nextafter(mv[f], np.float32(0)), np.nextafter(mv[f], np.float32(1e9)), 2 * mv[f], -1, np.nan, np.inf,
                -np.inf]
        for k in (1, 2, 17, 100, 128, 200, 254, 255):
            v = np.float32(k) * mv[f] / np.float32(255)
            vals += [np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(1e9))]
        x[f].reshape(-1)[:len(vals)] = np.array(vals, np.float32)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    return x, mv, lut


@pytest.mark.parametrize("d", [0, 5])
def test_colorize_random_table_two_ranges(eng, d):
    import torch
    x, mv, lut = _cmap_data(4)
    want = np.stack([VR.colorize(x[f], mv[f], lut, d) for f in range(2)])
    got = _np(eng.colorize(_t(eng, x), _t(eng, mv), _t(eng, lut), dilation=d))
    assert got.dtype == np.uint8 and np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    host = np.full(want.shape, SENTINEL, np.uint8)
    _lib.check(eng.lib.vppx_colorize_host(eng.ctx.handle, 2, 21, 67, _lib.np_ptr(x), _lib.np_ptr(mv), _lib.np_ptr(lut), d, _lib.np_ptr(host)))
    assert np.array_equal(host, want)
    tx, tm, tl = _t(eng, x), _t(eng, mv), _t(eng, lut)
    dev = torch.full(want.shape, SENTINEL, dtype=torch.uint8, device=eng.device)
    eng._bind_stream()
    _lib.check(eng.lib.vppx_colorize_dev(eng.ctx.handle, 2, 21, 67, tx.data_ptr(), tm.data_ptr(), tl.data_ptr(), d, dev.data_ptr()))
    assert np.array_equal(_np(dev), want)


def test_colorize_where_the_reference_is_undefined(eng):
    """max_val not > 0 (0, negative, NaN, -inf): index 0 everywhere, as the header says."""
    x, _, lut = _cmap_data(5)
    x = np.concatenate([x, x])
    mv = np.array([0, -3, np.nan, -np.inf], np.float32)
    got = _np(eng.colorize(_t(eng, x), _t(eng, mv), _t(eng, lut)))
    assert (got == lut[0]).all()
    for f in range(4):
        assert np.array_equal(got[f], VR.colorize(x[f], mv[f], lut))


def test_finite_max_and_the_colour_map_it_feeds(eng):
    rng = np.random.default_rng(6)
    x = rng.uniform(-50, 190, (5, 33, 130)).astype(np.float32)
    x[0, 3, 4], x[0, 5, 6] = np.inf, -np.inf
    x[1] = -np.abs(x[1])
    x[1, 0, 0] = np.inf                     # all else negative: the maximum is a negative number, not +inf
    x[2] = np.inf
    x[2, 1::2] = -np.inf                    # nothing finite: -inf
    x[3, -1, -1] = 1000                     # the last pixel counts
    x[4, 7, 7] = np.nan                     # torch's max propagates NaN
    got = _np(eng.finite_max(_t(eng, x)))
    assert got.dtype == np.float32 and got.shape == (5,)
    for f in range(4):
        assert got[f] == VR.finite_max(x[f]), f
    assert got[2] == -np.inf and got[3] == 1000 and np.isnan(got[4])
    import torch
    want = torch.where(torch.isinf(torch.from_numpy(x[0])), -float('inf'), torch.from_numpy(x[0])).max()   # test.py:318
    assert got[0] == want.item()
    big = rng.uniform(0, 190, (2, 540, 960)).astype(np.float32)      # more than one block per frame
    big[0, 539, 959] = 200
    big[1, 300, 17] = np.inf
    got = _np(eng.finite_max(_t(eng, big)))
    assert got[0] == 200 and got[1] == VR.finite_max(big[1])
    # and through the colour map, as test.py:318-343 chains them
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    xs = _t(eng, x[:2])
    pic = _np(eng.colorize(xs, eng.finite_max(xs), _t(eng, lut), dilation=2))
    for f in range(2):
        assert np.array_equal(pic[f], VR.colorize(x[f], VR.finite_max(x[f]), lut, 2))


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_leave_out_untouched(eng):
    import torch
    lib, h = eng.lib, eng.ctx.handle
    B, H, W = 1, 6, 9
    a = np.ones((B, H, W), np.float32)
    ta = _t(eng, a)
    lut = np.zeros((256, 3), np.uint8)
    tl = _t(eng, lut)
    mv = np.ones(1, np.float32)
    tm = _t(eng, mv)
    hout = np.full((6, B, H, W, 3), SENTINEL, np.uint8)
    dout = torch.full((6, B, H, W, 3), SENTINEL, dtype=torch.uint8, device=eng.device)
    pa, po, da, do = a.ctypes.data, hout.ctypes.data, ta.data_ptr(), dout.data_ptr()
    INV, UNS = -1, -10
    eng._bind_stream()

    def refused(rc, code, word):
        assert rc == code, (rc, code, word)
        assert word in lib.vppx_last_error().decode(), (word, lib.vppx_last_error())

    for fn, x, o in ((lib.vppx_error_colors_host, pa, po), (lib.vppx_error_colors_dev, da, do)):
        refused(fn(h, B, H, W, None, None, 1.0, 1, 1, o), INV, "NULL")
        refused(fn(h, B, H, W, x, None, 1.0, 1, 1, None), INV, "NULL")
        refused(fn(h, 0, H, W, x, None, 1.0, 1, 1, o), INV, "shape")
        refused(fn(h, B, -1, W, x, None, 1.0, 1, 1, o), INV, "shape")
        refused(fn(h, B, H, 0, x, None, 1.0, 1, 1, o), INV, "shape")
        refused(fn(h, B, H, W, x, None, 1.0, 1, -1, o), INV, "dilation")
        refused(fn(h, B, H, W, x, None, 0.0, 1, 1, o), INV, "scale")
        refused(fn(h, B, H, W, x, None, -2.0, 1, 1, o), INV, "scale")
        refused(fn(h, B, H, W, x, None, float("nan"), 1, 1, o), INV, "scale")
        refused(fn(h, B, H, W, x, None, 1.0, 1, _lib.VIZ_MAX_DILATION + 1, o), UNS, str(_lib.VIZ_MAX_DILATION))
    for fn, x, o in ((lib.vppx_guided_visualize_host, pa, po), (lib.vppx_guided_visualize_dev, da, do)):
        refused(fn(h, B, H, W, x, x, None, 1.0, 7, 63, o), INV, "NULL")
        refused(fn(h, B, H, W, None, x, x, 1.0, 7, 63, o), INV, "NULL")
        refused(fn(h, B, H, W, x, x, x, 1.0, 7, 63, None), INV, "NULL")
        refused(fn(h, B, 0, W, x, x, x, 1.0, 7, 63, o), INV, "shape")
        refused(fn(h, B, H, W, x, x, x, 1.0, -7, 63, o), INV, "dilation")
        refused(fn(h, B, H, W, x, x, x, 1.0, 7, 0, o), INV, "which")
        refused(fn(h, B, H, W, x, x, x, 1.0, 7, 64, o), INV, "which")
        refused(fn(h, B, H, W, x, x, x, 0.0, 7, 63, o), INV, "scale")
        refused(fn(h, B, H, W, x, x, x, 1.0, _lib.VIZ_MAX_DILATION + 1, 63, o), UNS, str(_lib.VIZ_MAX_DILATION))
    for fn, x, m, l, o in ((lib.vppx_colorize_host, pa, mv.ctypes.data, lut.ctypes.data, po),
                           (lib.vppx_colorize_dev, da, tm.data_ptr(), tl.data_ptr(), do)):
        refused(fn(h, B, H, W, x, None, l, 0, o), INV, "NULL")
        refused(fn(h, B, H, W, x, m, None, 0, o), INV, "NULL")
        refused(fn(h, B, H, -3, x, m, l, 0, o), INV, "shape")
        refused(fn(h, B, H, W, x, m, l, -1, o), INV, "dilation")
        refused(fn(h, B, H, W, x, m, l, _lib.VIZ_MAX_DILATION + 1, o), UNS, str(_lib.VIZ_MAX_DILATION))
    refused(lib.vppx_finite_max_dev(h, B, H, W, None, do), INV, "NULL")
    refused(lib.vppx_finite_max_dev(h, B, H, W, da, None), INV, "NULL")
    refused(lib.vppx_finite_max_dev(h, 0, H, W, da, do), INV, "shape")
    assert (hout == SENTINEL).all() and (_np(dout) == SENTINEL).all()
    # the Engine refuses the same before it calls the library
    for kw in (dict(dilation=-1), dict(dilation=_lib.VIZ_MAX_DILATION + 1), dict(scale=0), dict(which=0), dict(which="mae")):
        with pytest.raises(ValueError):
            eng.guided_visualize(ta, ta, ta, out=dout, **kw)
    with pytest.raises(ValueError):
        eng.error_colors(ta, mask=ta[:, :3])
    assert (_np(dout) == SENTINEL).all()
    # and the context still works
    assert np.array_equal(_np(eng.error_colors(ta)), _ref_errors(a, None, 1, True, 1))


# ---------------------------------------------------------------------------------------------------------------------
# the one full-size case
# ---------------------------------------------------------------------------------------------------------------------
def test_full_size_two_frames_dilation_7(eng):
    disp, gt, valid = _data(2, 540, 960, seed=540)
    _check_guided(eng, disp, gt, valid, 1, 7, "540x960")
    e = _err_of(disp, gt)
    got = _np(eng.error_colors(_t(eng, e), _t(eng, (gt > 0).astype(np.float32)), dilation=7))      # test.py:327
    assert np.array_equal(got, _ref_errors(e, gt > 0, 1, True, 7))
