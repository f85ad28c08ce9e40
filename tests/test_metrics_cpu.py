"""CPU-side checks of the evaluation-metrics layer (losses.guided_metrics on the device, include/vppx.h "evaluation metrics"):
the new symbols are declared, exported and bound; the structs have the sizes the header states; without a context the host
entry point fails loudly; the Python wrappers refuse what the library would refuse before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vppstereo_amd import _lib, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vppx_eval_params_default", "vppx_guided_metrics_dev", "vppx_guided_metrics_host", "vppx_occ_vpp_rsgm_eval_dev",
       "vppx_fstream_create_eval", "vppx_fstream_push_eval", "vppx_fstream_pop_eval"]


def test_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "vppx.h")).read()
    declared = set(re.findall(r"\b(vppx_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert "#define VPPX_FS_METRICS 16" in hdr and "#define VPPX_FS_NO_DISP 32" in hdr
    assert (_lib.FS_METRICS, _lib.FS_NO_DISP) == (16, 32)
    assert re.search(r"guided_metrics\(\)\s+losses\.py:13-24", hdr)
    assert lib.vppx_version() == 100


def test_struct_sizes_and_defaults():
    assert C.sizeof(_lib.VppxMetrics) == 64 and C.sizeof(_lib.VppxEvalParams) == 8
    assert C.sizeof(_lib.VppxVppParams) == 104 and C.sizeof(_lib.VppxRsgmParams) == 32
    p = _lib.VppxEvalParams(gt_scale=77, reserved0=5)
    _lib.load().vppx_eval_params_default(C.byref(p))
    assert (p.gt_scale, p.reserved0) == (1, 0)
    assert _lib.eval_params(gt_scale=3).gt_scale == 3
    with pytest.raises(TypeError, match="reserved0"):
        _lib.eval_params(reserved0=1)


def test_the_header_states_the_struct_sizes_a_c_compiler_sees(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "vppx.h"\nint main(void) { printf("%d %d %d %d\\n", (int)sizeof(VppxMetrics), '
                   '(int)sizeof(VppxEvalParams), (int)sizeof(VppxVppParams), (int)sizeof(VppxRsgmParams)); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.check_output([exe], text=True).split() == ["64", "8", "104", "32"]


def test_host_entry_point_without_a_context_fails_with_a_message():
    lib = _lib.load()
    d = np.zeros((1, 4, 4), np.float32)
    rec = _lib.VppxMetrics()
    rc = lib.vppx_guided_metrics_host(C.c_void_p(), None, 1, 4, 4, d.ctypes.data, 4, 4, d.ctypes.data, d.ctypes.data, C.byref(rec), None)
    assert rc == -7 and b"context is NULL" in lib.vppx_last_error()
    rc = lib.vppx_guided_metrics_dev(C.c_void_p(), None, 1, 4, 4, None, 4, 4, None, None, None, None)
    assert rc == -7 and b"context is NULL" in lib.vppx_last_error()
    rc = lib.vppx_fstream_push_eval(C.c_void_p(), None, None, None, None, None, None, None)
    assert rc == -1 and b"stream is NULL" in lib.vppx_last_error()


def test_wrappers_refuse_bad_ground_truth_before_they_touch_the_device():
    l = np.zeros((30, 64, 3), np.uint8)
    h = np.zeros((30, 64), np.float32)
    with pytest.raises(ValueError, match="go together"):
        pipeline.run_frame(l, l, h, gt=h)
    with pytest.raises(ValueError, match="go together"):
        pipeline.run_frame(l, l, h, validgt=h)
    with pytest.raises(ValueError, match="return_errormap"):
        pipeline.run_frame(l, l, h, return_errormap=True)
    with pytest.raises(ValueError, match="expected shape"):
        pipeline.run_frame(l, l, h, gt=h[:-1], validgt=h[:-1])
    # --iscale 2 --oscale 1 on 375 rows returns a 374-row map: the full-size gt does not fit it (the reference dies in a broadcast)
    l2, h2 = np.zeros((375, 64, 3), np.uint8), np.zeros((375, 64), np.float32)
    with pytest.raises(ValueError, match="375 x 64 at gt_scale 1 is 375 x 64, the disparity map is 374 x 64"):
        pipeline.run_frame(l2, l2, h2, iscale=2, oscale=1, gt=h2, validgt=h2)
    # --oscale alone decimates the gt but not the map
    with pytest.raises(ValueError, match="gt_scale 2"):
        pipeline.run_frame(l, l, h, oscale=2, gt=h, validgt=h)
    with pytest.raises(ValueError, match="gt_scale 0"):
        _lib.check_gt_shape(8, 8, 0, 8, 8)
    _lib.check_gt_shape(375, 1242, 2, 187, 621)
    _lib.check_gt_shape(375, 1242, 3, 125, 414)


def test_stream_refuses_return_disp_false_without_metrics_before_it_opens_a_device():
    with pytest.raises(ValueError, match="metrics=True"):
        pipeline.FrameStream(32, 64, return_disp=False)
    with pytest.raises(ValueError, match="return_patterns"):
        pipeline.FrameStream(32, 64, metrics=True, return_disp=False, return_patterns=True)
    with pytest.raises(ValueError, match="374 x 64"):
        pipeline.FrameStream(375, 64, metrics=True, iscale=2, oscale=1)


def test_metrics_dict_has_the_references_keys():
    rec = _lib.VppxMetrics(0.5, 0.25, 0.125, 0.0, 1.5, 2.5, 8.0, 0.0)
    assert _lib.metrics_dict(rec) == {'bad 1.0': 0.5, 'bad 2.0': 0.25, 'bad 3.0': 0.125, 'bad 4.0': 0.0, 'avgerr': 1.5, 'rms': 2.5}
    assert _lib.metrics_dict([0.5, 0.25, 0.125, 0.0, 1.5, 2.5, 8.0, 0.0]) == _lib.metrics_dict(rec)


def test_copy_pool_mask_job_writes_one_byte_per_float(tmp_path):
    """The stream's validity plane: copy_pool.h kind 1 turns float32 validgt into `validgt > 0` bytes (NaN and negatives are 0)."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    src = tmp_path / "m.cpp"
    src.write_text('''#include <cstdio>
#include <cmath>
#include <vector>
#include "copy_pool.h"
int main() {
    const size_t n = 518400 + 3;
    std::vector<float> v(n);
    for (size_t i = 0; i < n; i++) v[i] = i % 5 == 0 ? 0.f : (i % 5 == 1 ? -1.f : (i % 5 == 2 ? 0.5f : (i % 5 == 3 ? NAN : 2.f)));
    for (int nt : {0, 3}) {
        vppx_host::CopyPool pool(nt);
        std::vector<unsigned char> d(n + 1, 9);
        vppx_host::CopyJob j[1] = {{d.data(), v.data(), n, 1}};
        pool.copy(j, 1);
        for (size_t i = 0; i < n; i++) if (d[i] != (unsigned char)(v[i] > 0.f)) { printf("BAD %zu\\n", i); return 1; }
        if (d[n] != 9) { printf("OVERRUN\\n"); return 1; }
    }
    printf("MASK_OK\\n");
    return 0;
}
''')
    exe = str(tmp_path / "m")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "vppstereo_amd", "csrc"), str(src), "-o", exe])
    assert "MASK_OK" in subprocess.check_output([exe], text=True)
