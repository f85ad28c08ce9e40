"""--iscale timing (test.py:136-148, :247-248 with the rSGM matcher): ms per `Engine.vpp_rsgm` call at iscale 1 and iscale 2
on the same full-size batch (540x960x192, 3 % hints, 32 frames, occlusion mask on the way), the two alternated call by call and
timed with device events after warm-up.  Writes one JSON object (median and all samples per iscale).

    python tools/scale_bench.py out.json [--H 540 --W 960 --D 192 --B 32 --p 0.03 --iters 10 --warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--H", type=int, default=540)
    ap.add_argument("--W", type=int, default=960)
    ap.add_argument("--D", type=int, default=192)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--p", type=float, default=0.03)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch
    import synth
    from vppstereo_amd import pipeline
    from vppstereo_amd.engine import Engine
    eng = Engine()
    dev = eng.device
    b = synth.make_batch(a.B, a.H, a.W, a.D, a.p, seed=5)
    left, right, hints = (torch.from_numpy(b[k]).to(dev) for k in ("left", "right", "hints"))
    outs = {}
    for s in (1, 2):
        _, _, Ho, Wo = pipeline.scaled_shape(a.H, a.W, s, 1)
        outs[s] = torch.empty((a.B, Ho, Wo), dtype=torch.float32, device=dev)

    def call(s):
        eng.vpp_rsgm(left, right, hints, g_occ="occlusion_heuristic", out=outs[s], seed=1, rsgm_kw=dict(dmax=a.D), iscale=s)

    for _ in range(a.warmup):
        for s in (1, 2):
            call(s)
    torch.cuda.synchronize()
    samples = {1: [], 2: []}
    for _ in range(a.iters):
        for s in (1, 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(s)
            e1.record()
            e1.synchronize()
            samples[s].append(round(e0.elapsed_time(e1), 4))
    eng.status()
    res = {"shape": [a.B, a.H, a.W, a.D], "p_hints": a.p, "iters": a.iters, "device": eng.ctx.device_name}
    for s in (1, 2):
        h, w, Ho, Wo = pipeline.scaled_shape(a.H, a.W, s, 1)
        res[f"iscale{s}"] = {"ms_median": float(np.median(samples[s])), "ms_per_frame": float(np.median(samples[s])) / a.B,
                             "matcher_shape": [h, w], "out_shape": [Ho, Wo], "samples_ms": samples[s]}
    C = 3
    res["bytes"] = {"front_read": a.B * a.H * a.W * (2 * C + 4), "front_write": a.B * (a.H // 2) * (a.W // 2) * (2 * C + 4),
                    "restore_read": a.B * (a.H // 2) * (a.W // 2) * 4, "restore_write": a.B * Ho * Wo * 4}
    res["routes_iscale2"] = eng.last_routes()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "routes_iscale2"}))


if __name__ == "__main__":
    main()
