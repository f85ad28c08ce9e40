#!/usr/bin/env python3
"""tools/sample_stream.py [out.json] [--frames N] [--rounds R]: frames per second of the loop of test.py:291-311 for a dataset
without raw hints -- sample the hints from the ground truth (test.py:125-129), match, evaluate -- at 540x960x192 on an evaluating
frame stream, three ways on the same synthetic frames (synth.make_frame, gt = its dense ground truth, ~85 % of it valid),
occlusion mask on the way:
  (a) host_sample   torch `vppstereo_amd.losses.sample_hints` per frame on the host (one thread), then push_eval
  (b) presampled    the hints sampled beforehand, outside the timed loop, then push_eval: the rate of the stream without sampling
  (c) push_sampled  FrameStream(sample=p, metrics=True).push_sampled from gt: no hints plane goes up at all
The streams are open together and take turns, round after round, in one process on one device; every timed window is a whole
run() of N frames.  Reported: frames per second per round, the median over the rounds, per round (c) / (b), and (b)'s own spread.

  --batched [--rounds R]   instead: the batched step, 32 x 540x960x192 with occlusion_heuristic, pipelined, resident inputs:
                           Engine.vpp_rsgm(sample=...) against the same call on resident pre-sampled hints, alternated legs
  --kernel B [--launches K] instead: K launches of the sampling kernel alone on B frames of 540x960 (for a kernel trace)"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import synth

arg = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
H, W, D = arg("--height", 540), arg("--width", 960), arg("--dmax", 192)
P = 0.05


def save(res):
    print(json.dumps(res), flush=True)
    path = [a for a in sys.argv[1:] if a.endswith(".json")]
    if path:
        json.dump(res, open(path[0], "w"), indent=1)


def kernel_only(B):
    import torch
    from vppstereo_amd.engine import Engine
    eng = Engine()
    g = torch.Generator().manual_seed(1)
    src = (torch.rand((B, H, W), generator=g) * 100 + 1).to(eng.device)
    valid = (torch.rand((B, H, W), generator=g) < 0.85).float().to(eng.device)
    out, vout = torch.empty_like(src), torch.empty_like(src)
    n = arg("--launches", 20)
    for k in range(2):      # the second pass is the timed one
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            eng.sample_hints(src, valid, P, 1 + i, out=out, valid_out=vout)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
    save({"what": "sampling kernel alone, back-to-back launches, host-timed", "frames": B, "shape": [H, W], "launches": n, "ms_per_launch": round(ms, 4),
          "selected_fraction": float(vout.mean())})


def batched():
    import torch
    from vppstereo_amd.engine import Engine
    B, rounds, steps = arg("--batch", 32), arg("--rounds", 5), arg("--steps", 12)
    eng = Engine()
    dev = eng.device
    b = synth.make_batch(8, H, W, D, 0.03, seed=900)
    idx = [i % 8 for i in range(B)]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a[idx])).to(dev)
    left, right, gt = T(b["left"]), T(b["right"]), T(b["gt"].astype(np.float32))
    vgt = (torch.rand((B, H, W), generator=torch.Generator().manual_seed(2)) < 0.85).float().to(dev)
    pre, _ = eng.sample_hints(gt, vgt, P, 1)
    outs = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(2)]
    occ = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    eng.set_pipeline(True)
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    ev.record()
    torch.cuda.synchronize()
    kw = dict(g_occ="occlusion_heuristic", occ_out=occ, seed=1, rsgm_kw=dict(dmax=D, subpixel=1), inputs_ready=ev)
    legs = {
        "presampled": lambda k: eng.vpp_rsgm(left, right, pre, out=outs[k & 1], **kw),
        "sampled": lambda k: eng.vpp_rsgm(left, right, out=outs[k & 1], sample=dict(probability=P, seed=1, src=gt, validsrc=vgt), **kw),
    }

    def window(name, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            legs[name](k)
        eng.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    for name in legs:
        window(name, 4)
    same = None
    legs["presampled"](0); eng.synchronize(); a = outs[0].clone()
    legs["sampled"](0); eng.synchronize(); same = bool(torch.equal(a, outs[0]))
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for name in legs:
            ms[name].append(round(window(name, steps), 4))
    res = {"what": "batched step, ms per step, pipelined, resident inputs; legs alternated in one process", "shape": [B, H, W, D],
           "steps_per_window": steps, "rounds": rounds, "parts": eng.last_call_parts(), "same_disparities": same, "ms_per_step": ms,
           "median": {k: statistics.median(v) for k, v in ms.items()},
           "presampled_spread": round(max(ms["presampled"]) - min(ms["presampled"]), 4),
           "sampled_minus_presampled_per_round": [round(s - p_, 4) for s, p_ in zip(ms["sampled"], ms["presampled"])]}
    res["sampled_minus_presampled_median"] = round(res["median"]["sampled"] - res["median"]["presampled"], 4)
    save(res)


def streams():
    import torch
    from vppstereo_amd import losses, pipeline
    n_frames, rounds, pool = arg("--frames", 1024), arg("--rounds", 5), 8
    torch.set_num_threads(1)
    frames = []
    for f in range(pool):
        fr = synth.make_frame(H, W, D, 0.03, seed=900 + f)
        vgt = (np.random.default_rng(f).random((H, W)) < 0.85).astype(np.float32)
        gt = np.ascontiguousarray(fr["gt"], np.float32)
        torch.manual_seed(f)
        pre = losses.sample_hints(torch.from_numpy(gt), torch.from_numpy(vgt) > 0, P)[0].numpy()
        frames.append((fr["left"], fr["right"], gt, vgt, pre))
    kw = dict(maskocc=True, rsgm_kw=dict(dmax=D), seed=1, metrics=True)
    fss = {"host_sample": pipeline.FrameStream(H, W, 3, **kw), "presampled": pipeline.FrameStream(H, W, 3, **kw),
           "push_sampled": pipeline.FrameStream(H, W, 3, sample=P, **kw)}
    host_s = [0.0]

    def gen(name, n):
        for i in range(n):
            l, r, gt, vgt, pre = frames[i % pool]
            if name == "push_sampled":
                yield (l, r, None, None, None, gt, vgt)
            elif name == "presampled":
                yield (l, r, pre, None, None, gt, vgt)
            else:
                t = time.perf_counter()
                h = losses.sample_hints(torch.from_numpy(gt), torch.from_numpy(vgt) > 0, P)[0].numpy()
                host_s[0] += time.perf_counter() - t
                yield (l, r, h, None, None, gt, vgt)

    def run(name, n):
        acc, k = 0.0, 0
        for r in fss[name].run(gen(name, n)):
            acc += r[1]["avgerr"] + float(r[0][0, 0])
            k += 1
        assert k == n
        return acc
    res = {"what": "sample + match + evaluate loop, frames per second (pageable numpy in, disparities + metrics out), three variants "
                   "alternated in one process", "shape": [H, W, D], "probability": P, "frames_per_window": n_frames, "rounds": rounds,
           "batch": fss["presampled"].batch, "depth": fss["presampled"].depth, "fps": {k: [] for k in fss}}
    try:
        for name in fss:
            run(name, fss[name].batch * 4)
        host_s[0] = 0.0
        for _ in range(rounds):
            for name in fss:
                n = n_frames if name != "host_sample" else max(fss[name].batch * 4, n_frames // 8)   # (a) is ~25 times slower per frame
                t0 = time.perf_counter()
                run(name, n)
                res["fps"][name].append(round(n / (time.perf_counter() - t0), 1))
        res["host_sample_hints_ms_per_frame"] = round(host_s[0] / (rounds * max(fss["host_sample"].batch * 4, n_frames // 8)) * 1e3, 3)
        res["reruns"] = {k: s.counts()[3] for k, s in fss.items()}
    finally:
        for s in fss.values():
            s.close()
    f = res["fps"]
    res["fps_median"] = {k: statistics.median(v) for k, v in f.items()}
    res["ms_per_frame_median"] = {k: round(1e3 / v, 4) for k, v in res["fps_median"].items()}
    res["sampled_over_presampled_per_round"] = [round(c / b, 4) for c, b in zip(f["push_sampled"], f["presampled"])]
    res["presampled_spread_fraction"] = round((max(f["presampled"]) - min(f["presampled"])) / statistics.median(f["presampled"]), 4)
    res["sampled_over_host_median"] = round(res["fps_median"]["push_sampled"] / res["fps_median"]["host_sample"], 2)
    save(res)


if __name__ == "__main__":
    if "--kernel" in sys.argv:
        kernel_only(arg("--kernel", 32))
    elif "--batched" in sys.argv:
        batched()
    else:
        streams()
