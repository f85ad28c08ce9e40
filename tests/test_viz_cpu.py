"""CPU-side checks of the picture layer (include/vppx.h "pictures": utils.py:17-79, test.py:318-343 on the device):
tests/_viz_ref.py, the numpy restatement the GPU tests compare against, reproduces the reference's own output
(tests/golden/viz_cases.npz) byte for byte and its dilation agrees with a brute-force double loop; the new symbols are
declared, exported and bound; vppstereo_amd.utils has the reference's signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import _viz_ref as VR
from vppstereo_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vppx_error_colors_dev", "vppx_error_colors_host", "vppx_guided_visualize_dev", "vppx_guided_visualize_host",
       "vppx_colorize_dev", "vppx_colorize_host", "vppx_finite_max_dev"]


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "viz_cases.npz"))


def test_ref_error_colors_reproduce_the_reference(cases):
    n = 0
    for scale in (1, 3, 19):
        for bgr in (True, False):
            for dil in (0, 1):
                for mname in ("none", "mask", "mask2"):
                    mask = None if mname == "none" else cases["ce_" + mname]
                    want = cases[f"ce_out_s{scale}_b{int(bgr)}_d{dil}_{mname}"]
                    got = VR.error_colors(cases["ce_errors"], scale, mask, bgr, dil)
                    assert got.dtype == np.uint8 and got.shape == want.shape
                    assert np.array_equal(got, want), (scale, bgr, dil, mname)
                    n += 1
    assert n == 36


def test_golden_inputs_cover_the_edges(cases):
    """The fixture is only worth something if the edge values are in it and take different colours on their two sides."""
    sp = cases["special"]
    e = cases["ce_errors"].reshape(-1)
    assert np.array_equal(e[:len(sp)], sp, equal_nan=True)
    for edge in (0.1875, 0.375, 0.75, 1.5, 3, 6, 12, 24, 48):
        for v in (np.float32(edge), np.nextafter(np.float32(edge), np.float32(0)), np.nextafter(np.float32(edge), np.float32(99)),
                  np.float32(edge / 3), np.float32(edge / 19)):
            assert (sp == v).any(), edge
    assert np.isnan(sp).any() and np.isinf(sp).any()
    # every edge / 3 is exact; scale 19 is where comparing in double matters: float32(edge / 19) lies below edge / 19, so a
    # comparison in float32 would put it into the higher bin
    assert all(float(np.float32(edge / 19)) < edge / 19 for edge in (0.1875, 0.375, 0.75, 1.5, 3, 6, 12, 24, 48))
    e32 = cases["ce_errors"].reshape(-1)[:len(sp)]
    nineteen = cases["ce_out_s19_b1_d1_none"].reshape(-1, 3)[:len(sp)]
    with np.errstate(invalid="ignore"):
        in_f32 = np.zeros((len(sp), 3), np.uint8)
        for row in VR.COLOR_MAP:
            in_f32[(e32 >= np.float32(row[0] / 19)) & (e32 <= np.float32(row[1] / 19))] = row[2:].astype(np.uint8)
    assert not np.array_equal(in_f32, nineteen)
    assert set(np.unique(cases["gv_valid"])) == {-1.0, 0.0, 0.5, 1.0}
    d, g = cases["gv_disp"], cases["gv_gt"]
    assert np.isnan(d).any() and np.isnan(g).any() and np.isposinf(d).any() and np.isneginf(d).any() and np.isinf(g).any()
    one = cases["ce_out_s1_b1_d1_none"].reshape(-1, 3)
    three = cases["ce_out_s3_b1_d1_none"].reshape(-1, 3)
    for pic in (one, three, nineteen):
        assert len(np.unique(pic[:len(sp)], axis=0)) == 11  # ten bins and black


def test_ref_guided_visualize_reproduces_the_reference(cases):
    for scale in (1, 3, 19):
        for dil in (0, 1):
            want = cases[f"gv_out_s{scale}_d{dil}"]
            got = VR.guided_visualize(cases["gv_disp"], cases["gv_gt"], cases["gv_valid"], scale, dil)
            assert tuple(got) == VR.KEYS == _lib.VIZ_KEYS
            for n, k in enumerate(VR.KEYS):
                assert np.array_equal(got[k], want[n]), (scale, dil, k)


@pytest.mark.parametrize("d", [2, 3, 4, 7])
def test_ref_dilation_against_brute_force(d):
    rng = np.random.default_rng(d)
    img = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    img[rng.random((6, 7)) < 0.5] = 0
    assert np.array_equal(VR.dilate(img, d), VR.dilate_brute(img, d))
    # a single bright pixel spreads over exactly the window: up / left d//2, down / right d-1-d//2
    one = np.zeros((6, 7, 3), np.uint8)
    one[3, 3] = (9, 8, 7)
    out = VR.dilate(one, d)
    ys, xs = np.nonzero(out[..., 0])
    a = d // 2
    assert ys.min() == max(0, 3 - (d - 1 - a)) and ys.max() == min(5, 3 + a)
    assert xs.min() == max(0, 3 - (d - 1 - a)) and xs.max() == min(6, 3 + a)


def test_ref_dilation_identity():
    img = np.arange(6 * 7 * 3, dtype=np.uint8).reshape(6, 7, 3)
    for d in (0, 1):
        assert np.array_equal(VR.dilate(img, d), img)


def test_ref_colorize_and_finite_max():
    lut = np.arange(768, dtype=np.uint32).reshape(256, 3).astype(np.uint8)
    x = np.array([[0, 5, 10, 20, -3, np.nan, np.inf, -np.inf, 9.999]], np.float32)
    idx = [0, 127, 255, 255, 0, 0, 255, 0, int(np.float32(9.999) / np.float32(10) * np.float32(255))]
    assert np.array_equal(VR.colorize(x, 10, lut), lut[idx][None])
    assert np.array_equal(VR.colorize(x, 0, lut), np.broadcast_to(lut[0], (1, 9, 3)))
    assert np.array_equal(VR.colorize(x, np.nan, lut), np.broadcast_to(lut[0], (1, 9, 3)))
    assert VR.finite_max(np.array([[1, np.inf, -np.inf, 7, -2]], np.float32)) == 7
    assert VR.finite_max(np.array([[np.inf, -np.inf]], np.float32)) == -np.inf


def test_new_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "vppx.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.argtypes[0] is C.c_void_p
    assert re.search(r"color_error_image_kitti\(\)\s+utils\.py:17-36", hdr)
    assert re.search(r"guided_visualize\(\)\s+utils\.py:39-79", hdr)
    m = re.search(r"#define\s+VPPX_VIZ_MAX_DILATION\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.VIZ_MAX_DILATION >= 15
    assert re.search(r"VPPX_VIZ_ALL\s*=\s*63", hdr) and _lib.VIZ_ALL == 63


def test_calls_without_a_context_fail_with_no_device():
    """There is no CPU fallback: a NULL context is VPPX_E_NO_DEVICE from every new entry point, and `out` is not written."""
    lib = _lib.load()
    a = np.zeros((4, 4), np.float32)
    out = np.full((6, 4, 4, 3), 0xA5, np.uint8)
    p, o = a.ctypes.data, out.ctypes.data
    null = C.c_void_p()
    assert lib.vppx_error_colors_host(null, 1, 4, 4, p, None, 1.0, 1, 1, o) == -7
    assert lib.vppx_error_colors_dev(null, 1, 4, 4, p, None, 1.0, 1, 1, o) == -7
    assert lib.vppx_guided_visualize_host(null, 1, 4, 4, p, p, p, 1.0, 7, 63, o) == -7
    assert lib.vppx_guided_visualize_dev(null, 1, 4, 4, p, p, p, 1.0, 7, 63, o) == -7
    assert lib.vppx_colorize_host(null, 1, 4, 4, p, p, o, 0, o) == -7
    assert lib.vppx_colorize_dev(null, 1, 4, 4, p, p, o, 0, o) == -7
    assert lib.vppx_finite_max_dev(null, 1, 4, 4, p, p) == -7
    assert (out == 0xA5).all()


def test_dropin_has_the_reference_signatures():
    from vppstereo_amd import utils as U
    import vppstereo_amd
    sig = inspect.signature(U.color_error_image_kitti)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("errors", inspect.Parameter.empty), ("scale", 1), ("mask", None), ("BGR", True), ("dilation", 1)]
    sig = inspect.signature(U.guided_visualize)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("disp", inspect.Parameter.empty), ("gt", inspect.Parameter.empty), ("valid", inspect.Parameter.empty), ("scale", 1),
        ("dilation", 7)]
    assert "vppstereo_amd.utils" in vppstereo_amd.__doc__


def test_which_selection():
    assert _lib.viz_which(None) == 63
    assert _lib.viz_which("avgerr") == 16
    assert _lib.viz_which(["bad 1.0", "rms"]) == 33
    assert _lib.viz_which(5) == 5
    for bad in (0, 64, "mae", []):
        with pytest.raises(ValueError):
            _lib.viz_which(bad)
