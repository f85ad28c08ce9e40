"""--iscale / --oscale, the parts that need no GPU: the C declarations and exports, the parameter helper, the Python signatures,
the scaled / restored shapes against torch's own F.interpolate on the CPU, and self-checks of the numpy restatement of the resize
(tests/_scale_ref.py, DESIGN section 5 rule 1)."""
import ctypes as C
import inspect
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _scale_ref as ref  # noqa: E402

NEW = ("vppx_scale_params_default", "vppx_scaled_shape", "vppx_occ_vpp_rsgm_scaled_dev", "vppx_occ_vpp_rsgm_scaled_host",
       "vppx_fstream_create_scaled")

C_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "vppx.h"

int main(void)
{
    VppxScaleParams sp;
    int h = 0, w = 0, Ho = 0, Wo = 0;
    vppx_scale_params_default(&sp);
    if (sp.iscale != 1 || sp.oscale != 1 || sizeof(VppxScaleParams) != 8) return 3;
    sp.iscale = 2;
    if (vppx_scaled_shape(375, 1242, &sp, &h, &w, &Ho, &Wo) != 0) return 4;
    if (h != 187 || w != 621 || Ho != 374 || Wo != 1242) return 5;
    sp.iscale = 0;
    if (vppx_scaled_shape(375, 1242, &sp, &h, &w, &Ho, &Wo) != VPPX_E_INVALID_ARG) return 6;
    (void)vppx_occ_vpp_rsgm_scaled_dev;
    (void)vppx_occ_vpp_rsgm_scaled_host;
    (void)vppx_fstream_create_scaled;
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_a_c99_program_using_the_scale_declarations_compiles_and_runs(tmp_path):
    src = tmp_path / "scale.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "scale"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "vppstereo_amd"), "-l:libvppx.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "vppstereo_amd")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


def test_the_header_declares_and_the_library_exports_the_scale_entry_points():
    from vppstereo_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "vppx.h")) as f:
        hdr = f.read()
    assert "typedef struct VppxScaleParams {" in hdr and "} VppxScaleParams;" in hdr
    body = hdr.split("typedef struct VppxScaleParams {")[1].split("} VppxScaleParams;")[0]
    assert [l.split("/*")[0].split() for l in body.strip().splitlines()] == [["int32_t", "iscale;"], ["int32_t", "oscale;"]]
    for name in NEW:
        assert name + "(" in hdr, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name


def test_scale_params_defaults_size_and_unknown_keywords():
    from vppstereo_amd import _lib
    p = _lib.scale_params()
    assert (p.iscale, p.oscale) == (1, 1)
    assert C.sizeof(_lib.VppxScaleParams) == 8
    q = _lib.scale_params(iscale=3, oscale=2)
    assert (q.iscale, q.oscale) == (3, 2)
    with pytest.raises(TypeError):
        _lib.scale_params(scale=2)
    with pytest.raises(TypeError):
        _lib.scale_params(iscale=2, blending=0.4)


def test_python_entry_points_take_the_scale_keywords():
    from vppstereo_amd import pipeline
    from vppstereo_amd.engine import Engine
    sig = inspect.signature(Engine.vpp_rsgm).parameters
    assert sig["iscale"].default == 1 and sig["oscale"].default == 1 and sig["disp_small"].default is None
    sig = inspect.signature(pipeline.run_frame).parameters
    assert sig["iscale"].default == 1 and sig["oscale"].default == 1
    sig = inspect.signature(pipeline.FrameStream.__init__).parameters
    assert sig["iscale"].default == 1 and sig["oscale"].default == 1
    sig = inspect.signature(pipeline.scaled_shape).parameters
    assert list(sig) == ["H", "W", "iscale", "oscale"]


def _torch_shapes(H, W, iscale, oscale):
    """test.py:142-148 and :247-248 on the CPU: the shape of the scaled hints and of the restored map."""
    import torch
    import torch.nn.functional as F
    hints = torch.zeros((1, 1, H, W))
    hs = F.interpolate(hints, scale_factor=1. / iscale, mode='nearest')
    h, w = hs.shape[-2:]
    assert (h, w) == (H // iscale, W // iscale)   # the resized pair, cv2.resize(..., (w // iscale, h // iscale))
    if iscale != 1 and iscale / oscale != 1:
        d = F.interpolate(hs[0][None], scale_factor=iscale / oscale, mode='nearest')
        return int(h), int(w), int(d.shape[-2]), int(d.shape[-1])
    return int(h), int(w), int(h), int(w)


@pytest.mark.parametrize("iscale", [1, 2, 3, 4])
@pytest.mark.parametrize("oscale", [1, 2, 3, 4])
def test_scaled_shape_equals_torch(iscale, oscale):
    from vppstereo_amd import pipeline
    for H, W in ((5 * iscale, 5 * iscale), (40, 96), (41, 97), (375, 1242), (540, 960), (37, 131), (1080, 1920), (99, 250)):
        if H // iscale < 1 or W // iscale < 1:
            continue
        assert pipeline.scaled_shape(H, W, iscale, oscale) == _torch_shapes(H, W, iscale, oscale), (H, W)


def test_scaled_shape_rejects_bad_factors():
    from vppstereo_amd import _lib, pipeline
    for i, o in ((0, 1), (1, 0), (-2, 1), (2, -1)):
        with pytest.raises(_lib.VppxError) as e:
            pipeline.scaled_shape(100, 100, i, o)
        assert e.value.code == -1 and "positive" in str(e.value)
    with pytest.raises(_lib.VppxError):
        pipeline.scaled_shape(3, 100, 4, 1)


def test_restatement_at_exactly_2x_equals_the_area_fast_path():
    rng = np.random.default_rng(1)
    for shape in ((40, 96, 3), (36, 50, 1), (8, 8, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        H, W = shape[:2]
        a = ref.resize_u8(img, W // 2, H // 2)
        b = ref.area_fast_2x(img)
        assert np.array_equal(a, b), shape
    # the formula by hand on one 2x2 block
    img = np.array([[10, 201], [33, 250]], np.uint8)
    assert int(ref.resize_u8(img, 1, 1)[0, 0]) == (10 + 201 + 33 + 250 + 2) >> 2


@pytest.mark.parametrize("s", [3, 5])
def test_restatement_at_an_odd_divisible_scale_picks_the_centre_pixel(s):
    rng = np.random.default_rng(s)
    img = rng.integers(0, 256, (7 * s, 9 * s, 3), dtype=np.uint8)
    out = ref.resize_u8(img, 9, 7)
    assert np.array_equal(out, img[s // 2::s, s // 2::s])


def test_restatement_tables_for_one_odd_width_by_hand():
    """W = 7 -> w = 3 (s = 2, scale_x = 7 / 3): fx = (dx + 0.5) * 7/3 - 0.5 = 2/3, 3, 16/3 -> (sx, fx) = (0, 0.6667), (3, 0),
    (5, 0.3333); weights cvRound((1 - fx) * 2048) / cvRound(fx * 2048) = 683 / 1365, 2048 / 0, 1365 / 683."""
    s0, s1, w0, w1 = ref.axis_table(7, 3)
    assert s0.tolist() == [0, 3, 5] and s1.tolist() == [1, 4, 6]
    assert w0.tolist() == [683, 2048, 1365] and w1.tolist() == [1365, 0, 683]
    row = np.array([[0, 30, 60, 90, 120, 150, 180]], np.uint8)
    # one row: t = S[sx] * a0 + S[sx + 1] * a1, then the vertical pass with b0 = 2048 (H = 1 -> h = 1 is the identity row)
    s0y, s1y, b0, b1 = ref.axis_table(1, 1)
    assert (s0y[0], s1y[0], b0[0], b1[0]) == (0, 0, 2048, 0)
    t = [0 * 683 + 30 * 1365, 90 * 2048, 150 * 1365 + 180 * 683]
    want = [(((2048 * (v >> 4)) >> 16) + 2) >> 2 for v in t]
    assert ref.resize_u8(row, 3, 1)[0].tolist() == want == [20, 90, 160]
