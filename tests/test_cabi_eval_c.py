"""The evaluating frame stream from PLAIN C (tests/c/fstream_eval_demo.c): strict C99 against include/vppx.h alone; without a GPU
it fails loudly (no CPU fallback); on the GPU it prints, per frame, the VppxMetrics record `pipeline.FrameStream(metrics=True)`
returns for the same frames -- as bytes -- with no disparity map copied out (VPPX_FS_NO_DISP)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_cabi_c import _has_gpu, _lcg_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "fstream_eval_demo.c")
LIBDIR = os.path.join(ROOT, "vppstereo_amd")


def _build(tmp_path):
    exe = str(tmp_path / "fstream_eval_demo")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", LIBDIR, "-lvppx", "-Wl,-rpath," + LIBDIR])
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_eval_demo_is_c99_links_and_fails_loudly_without_a_gpu(tmp_path):
    exe = _build(tmp_path)
    if _has_gpu():
        pytest.skip("checks the no-GPU failure mode")
    r = subprocess.run([exe, "2", "32", "64", "64", "2", "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr and "-7" in r.stderr and r.stdout == ""


def _lcg_gt(n, H, W):
    """gt / validgt as tests/c/fstream_eval_demo.c draws them: H * W more draws of the frame's LCG behind left, right and hints."""
    out = []
    for f in range(n):
        x = (12345 + 977 * f) & 0xFFFFFFFF
        skip = H * W * 3 * 2 + H * W
        a, c = 1664525, 1013904223
        # jump the affine map `skip` steps ahead by repeated squaring
        A, Cc, k = 1, 0, skip
        pa, pc = a, c
        while k:
            if k & 1:
                A, Cc = (pa * A) & 0xFFFFFFFF, (pa * Cc + pc) & 0xFFFFFFFF
            pa, pc = (pa * pa) & 0xFFFFFFFF, (pa * pc + pc) & 0xFFFFFFFF
            k >>= 1
        x = (A * x + Cc) & 0xFFFFFFFF
        r = np.empty(H * W, np.uint64)
        for i in range(H * W):
            x = (x * a + c) & 0xFFFFFFFF
            r[i] = x
        r = r.reshape(H, W)
        gt = (np.float32(3.0) + ((r >> np.uint64(16)) & np.uint64(15)).astype(np.float32) * np.float32(0.25)).astype(np.float32)
        valid = ((r >> np.uint64(30)) != 0).astype(np.float32)
        out.append((gt, valid))
    return out


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_c_program_prints_the_metrics_the_python_stream_returns(tmp_path):
    from vppstereo_amd.pipeline import FrameStream
    exe = _build(tmp_path)
    n, H, W, D, batch, seed = 7, 24, 48, 64, 3, 11
    r = subprocess.run([exe, str(n), str(H), str(W), str(D), str(batch), str(seed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    got = [line.split() for line in r.stdout.strip().splitlines()]
    assert [int(g[0]) for g in got] == list(range(n))
    frames = _lcg_frames(n, H, W)
    gts = _lcg_gt(n, H, W)
    recs = []
    with FrameStream(H, W, 3, batch=batch, seed=seed, maskocc=True, rsgm_kw=dict(dmax=D), metrics=True) as fs:
        for res in fs.run((l, r_, h, None, None, g, v) for (l, r_, h), (g, v) in zip(frames, gts)):
            disp, md = res
            recs.append(fs.last_metrics_record.copy())
            assert md['avgerr'] == recs[-1][4]
    for f in range(n):
        words = np.array([int(w, 16) for w in got[f][1:9]], np.uint64)
        assert words.tobytes() == recs[f].tobytes(), (f, got[f], recs[f])
        assert recs[f][6] > 0 and np.isfinite(recs[f][:6]).all(), f
    assert len({tuple(g[1:]) for g in got}) > 1
