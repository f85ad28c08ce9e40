"""--guided timing (test.py:207-223 with the rSGM matcher): ms per call of

  * guided `vppx_rsgm_dev` (compute_rsgm with hints / validhints on a batch): whole call and its stages (vppx_enable_stage_timing);
  * `Engine.vpp_rsgm(validhints=...)` against the same call without validhints.

VPPX_LIB names another build of the library to time; it must export everything include/vppx.h declares.

Default shape 540x960x192, 3 % hints, B = 16; after warm-up, the median of `--iters` timed calls.  Writes one JSON object.

    python tools/guided_bench.py out.json [--H 540 --W 960 --D 192 --B 16 --p 0.03 --iters 10 --warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def _median_ms(fn, sync, iters, warmup):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--H", type=int, default=540)
    ap.add_argument("--W", type=int, default=960)
    ap.add_argument("--D", type=int, default=192)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--p", type=float, default=0.03)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch
    import synth
    from vppstereo_amd import _lib
    lib_path, lib = _lib.LIB_PATH, _lib.load()
    vp = C.c_void_p

    def chk(rc):
        if rc != 0:
            raise RuntimeError(lib.vppx_last_error().decode())

    B, H, W, D = a.B, a.H, a.W, a.D
    b = synth.make_batch(B, H, W, D, a.p, seed=7)
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    left, right, hints = t(b["left"]), t(b["right"]), t(b["hints"])
    valid = t((b["hints"] > 0).astype(np.float32))
    out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    res = dict(lib=os.path.relpath(lib_path, ROOT), shape=[B, H, W, D], p_hints=a.p,
               hint_fraction=float((b["hints"] > 0).mean()), iters=a.iters, warmup=a.warmup)

    ctx = vp()
    chk(lib.vppx_create(C.byref(ctx), 0))
    rp = _lib.VppxRsgmParams()
    lib.vppx_rsgm_params_default(C.byref(rp))
    rp.dmax = D
    ptr = lambda x: C.c_void_p(x.data_ptr())
    call = lambda: chk(lib.vppx_rsgm_dev(ctx, C.byref(rp), B, H, W, 3, ptr(left), ptr(left), ptr(right), ptr(hints), ptr(valid),
                                         ptr(out)))
    res["rsgm_dev_guided_ms"], res["rsgm_dev_guided_all_ms"] = _median_ms(call, lambda: chk(lib.vppx_synchronize(ctx)), a.iters, a.warmup)
    guided_out = out.cpu().numpy()
    # the stages of one more call (events between the stages: a little slower in total)
    chk(lib.vppx_enable_stage_timing(ctx, 1))
    stages = {}
    for _ in range(3):
        call()
        chk(lib.vppx_synchronize(ctx))
        ms = (C.c_float * 96)()
        n = lib.vppx_get_stage_ms(ctx, ms, 96)
        for i in range(max(n, 0)):
            name = lib.vppx_stage_name(i).decode()
            stages.setdefault(name, []).append(round(float(ms[i]), 4))
    chk(lib.vppx_enable_stage_timing(ctx, 0))
    res["rsgm_dev_guided_stage_ms"] = {k: float(np.median(v)) for k, v in stages.items() if any(v)}
    res["guided_out_crc"] = int(np.frombuffer(guided_out.tobytes(), np.uint32).astype(np.uint64).sum() % (1 << 32))

    from vppstereo_amd.engine import Engine
    eng = Engine(0)
    kw = dict(g_occ="occlusion_heuristic", out=out, seed=3, rsgm_kw=dict(dmax=D))
    sync = torch.cuda.synchronize
    res["vpp_rsgm_guided_ms"], res["vpp_rsgm_guided_all_ms"] = _median_ms(
        lambda: eng.vpp_rsgm(left, right, hints, validhints=valid, **kw), sync, a.iters, a.warmup)
    res["vpp_rsgm_unguided_ms"], res["vpp_rsgm_unguided_all_ms"] = _median_ms(
        lambda: eng.vpp_rsgm(left, right, hints, **kw), sync, a.iters, a.warmup)
    res["guided_over_unguided"] = res["vpp_rsgm_guided_ms"] / res["vpp_rsgm_unguided_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
