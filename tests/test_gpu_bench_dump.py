"""GPU: `bench.py --dump-outputs` writes what its timed path computed -- the disparities and the occlusion mask of the last
timed step equal one unpipelined call of the 8-path layout on the same synthetic inputs, bit for bit -- and the result line
reports the number of timed steps it was given.  A plain run's line carries the headline only; `--full` adds the side legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dump_is_what_the_timed_path_computed(tmp_path):
    import torch
    from vppstereo_amd.engine import Engine
    B, H, W, D, p = 4, 60, 112, 64, 0.04
    out_dir = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", str(B), "--shape", str(H), str(W), str(D), str(p), "--sustained-steps", "0",
                        "--cpu-frames", "0", "--dump-outputs", out_dir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    disp = np.load(os.path.join(out_dir, "disparity.npy"))
    occ = np.load(os.path.join(out_dir, "occlusion_mask.npy"))
    assert disp.dtype == np.float32 and disp.shape == (B, H, W) and occ.dtype == np.float32 and occ.shape == (B, H, W)

    old = os.environ.get("VPPX_VERT")
    os.environ["VPPX_VERT"] = "0"
    try:
        eng = Engine()
    finally:
        if old is None:
            os.environ.pop("VPPX_VERT")
        else:
            os.environ["VPPX_VERT"] = old
    b = synth.make_batch(B, H, W, D, p, seed=1234, frame0=0)   # bench.py's inputs for one rank
    left, right, hints = (torch.from_numpy(np.ascontiguousarray(b[k])).to(eng.device) for k in ("left", "right", "hints"))
    occ_want = torch.empty((B, H, W), dtype=torch.uint8, device=eng.device)
    want = eng.vpp_rsgm(left, right, hints, g_occ="occlusion_heuristic", occ_out=occ_want, seed=1,
                        rsgm_kw=dict(dmax=D, subpixel=1))
    eng.synchronize()
    assert np.array_equal(occ, occ_want.cpu().numpy().astype(np.float32))
    assert np.array_equal(disp, want.cpu().numpy())


def test_bench_full_adds_the_side_legs_a_plain_run_leaves_out():
    B, H, W, D, p = 4, 60, 112, 64, 0.04
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
           "--shape", str(H), str(W), str(D), str(p)]
    lines = []
    for extra in ([], ["--full", "--sustained-steps", "5", "--cpu-frames", "1", "--no-cpu-parallel"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    plain, full = lines
    for line in lines:
        assert line["unit"] == "Mdisparities/s" and line["higher_is_better"] is True and line["dtype"] == "u16"
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert abs(line["value"] - B * H * W * D / line["ms_per_step"] / 1e3) <= 0.01 * line["value"] + 0.1
    side = ("ms_per_step_unpipelined", "ms_per_step_sustained", "roofline", "pipeline_roofline", "ms_per_step_without_g_occ", "b1",
            "stage_ms", "cpu_baseline", "cpu_baseline_simd", "epe_vs_cpu_oracle")
    assert [k for k in side if k in plain] == []
    assert [k for k in side if full.get(k) is None] == []
    assert full["sustained_steps"] == 5 and full["roofline"]["kernel_ms"] > 0 and full["b1"]["ms_per_frame"] > 0
    assert full["epe_vs_cpu_oracle"] <= 1e-4     # the GPU's frame 0 against the CPU oracle's
