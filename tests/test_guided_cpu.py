"""--guided on the batched VPP + rSGM call and the frame stream, the parts that need no GPU: the new C declarations compile as
strict C99, the library exports them, and the Python entry points take the new keywords."""
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "vppstereo_amd")
NEW = ("vppx_occ_vpp_rsgm_guided_dev", "vppx_occ_vpp_rsgm_guided_host", "vppx_fstream_push_guided")

C_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "vppx.h"

int main(void)
{
    vppx_ctx *ctx = NULL;
    VppxOccParams op;
    VppxVppParams vp;
    VppxRsgmParams rp;
    vppx_fstream *fs = NULL;
    int rc;
    vppx_occ_params_default(&op);
    vppx_vpp_params_default(&vp);
    vppx_rsgm_params_default(&rp);
    if (vppx_create(&ctx, 0) != 0) {
        fprintf(stderr, "%s\n", vppx_last_error());
        return 1;
    }
    rc = vppx_occ_vpp_rsgm_guided_dev(ctx, &op, &vp, &rp, 1, 8, 8, 3, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    rc |= vppx_occ_vpp_rsgm_guided_host(ctx, NULL, &vp, &rp, 1, 8, 8, 3, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    rc |= vppx_fstream_create(ctx, NULL, &vp, &rp, 2, 3, 8, 8, 3, VPPX_FS_GUIDED | VPPX_FS_PATTERNS, 1, &fs);
    rc |= vppx_fstream_push_guided(fs, NULL, NULL, NULL, NULL, NULL);
    vppx_fstream_destroy(fs);
    vppx_destroy(ctx);
    return rc != 0 && VPPX_FS_GUIDED == 8 ? 2 : 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_a_c99_program_using_the_guided_declarations_compiles_strictly(tmp_path):
    src = tmp_path / "guided.c"
    src.write_text(C_PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "guided.o")])


def test_the_library_exports_the_guided_entry_points():
    from vppstereo_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert _lib.FS_GUIDED == 8
    with open(os.path.join(ROOT, "include", "vppx.h")) as f:
        hdr = f.read()
    assert "#define VPPX_FS_GUIDED 8" in hdr
    for name in NEW:
        assert name + "(" in hdr, name


def test_the_python_entry_points_take_the_guided_keywords():
    from vppstereo_amd import engine, pipeline
    rf = inspect.signature(pipeline.run_frame).parameters
    assert "validhints" in rf and rf["validhints"].default is None
    fs = inspect.signature(pipeline.FrameStream.__init__).parameters
    assert "guided" in fs and fs["guided"].default is False
    push = list(inspect.signature(pipeline.FrameStream.push).parameters)
    assert push[1:] == ["left", "right", "hints", "g_occ", "validhints"]
    vr = inspect.signature(engine.Engine.vpp_rsgm).parameters
    assert "validhints" in vr and vr["validhints"].default is None
    rs = inspect.signature(engine.Engine.rsgm).parameters
    assert rs["hints"].default is None and rs["validhints"].default is None
