#!/usr/bin/env python3
"""tools/eval_stream.py [out.json] [--frames N] [--rounds R]: frames per second of the evaluation loop of test.py:291-311, :251-252
-- one numpy frame in, the six numbers of losses.guided_metrics out -- at 540x960x192, four ways on the same synthetic frames
(synth.make_frame, gt = its dense ground truth, ~85 % of it valid), occlusion mask on the way:
  (a) host_metrics     FrameStream, then the numpy `vppstereo_amd.losses.guided_metrics` per popped frame on the host
  (b) device_metrics   FrameStream(metrics=True): gt + one byte of validity go up with the frame, 64 bytes more come down
  (c) metrics_only     FrameStream(metrics=True, return_disp=False): the disparity map never leaves the device
  (d) plain            FrameStream alone, no metrics at all (what the stream did before it could evaluate)
The four streams are open together and take turns, round after round, in one process on one device; every timed window is a whole
run() of N frames (pageable numpy in, fresh numpy / dicts out).  Reported: frames per second per round, the median over the rounds,
and per round the ratios (b) / (d) and (b) / (a)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import synth


def main():
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    n_frames, rounds, pool = arg("--frames", 1024), arg("--rounds", 5), 8
    H, W, D, p = arg("--height", 540), arg("--width", 960), arg("--dmax", 192), 0.03
    from vppstereo_amd import losses, pipeline
    frames = []
    for f in range(pool):
        fr = synth.make_frame(H, W, D, p, seed=900 + f)
        vgt = (np.random.default_rng(f).random((H, W)) < 0.85).astype(np.float32)
        frames.append((fr["left"], fr["right"], fr["hints"], fr["gt"], vgt))
    kw = dict(maskocc=True, rsgm_kw=dict(dmax=D), seed=1)
    make = {
        "host_metrics": lambda: pipeline.FrameStream(H, W, 3, **kw),
        "device_metrics": lambda: pipeline.FrameStream(H, W, 3, metrics=True, **kw),
        "metrics_only": lambda: pipeline.FrameStream(H, W, 3, metrics=True, return_disp=False, **kw),
        "plain": lambda: pipeline.FrameStream(H, W, 3, **kw),
    }
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None   # one variant alone, e.g. under a profiler
    streams = {k: f() for k, f in make.items() if only in (None, k)}
    # where the host's time goes, per variant: seconds inside push (the copies into the ring + a batch's submission) and inside
    # the native pop (waiting for the batch + the copy out); the rest of a window is Python and, for (a), the numpy metrics
    split = {k: [0.0, 0.0] for k in streams}
    for k, fs in streams.items():
        def wrap(fs=fs, tp=split[k]):
            push0, pop0 = fs.push, fs._pop_native

            def push1(*a, **b):
                t = time.perf_counter(); push0(*a, **b); tp[0] += time.perf_counter() - t

            def pop1():
                t = time.perf_counter(); r = pop0(); tp[1] += time.perf_counter() - t
                return r
            fs.push, fs._pop_native = push1, pop1
        wrap()

    def run(name, n):
        fs = streams[name]
        acc, k = 0.0, 0
        if name in ("host_metrics", "plain"):
            gen = (frames[i % pool][:3] for i in range(n))
            for i, d in enumerate(fs.run(gen)):
                if name == "host_metrics":
                    fr = frames[i % pool]
                    acc += float(losses.guided_metrics(d, fr[3], fr[4])["avgerr"])
                else:
                    acc += float(d[0, 0])      # the caller touches the result
                k += 1
        else:
            gen = ((fr[0], fr[1], fr[2], None, None, fr[3], fr[4]) for fr in (frames[i % pool] for i in range(n)))
            for r in fs.run(gen):
                acc += (r if name == "metrics_only" else r[1])["avgerr"]
                k += 1
        assert k == n
        return acc

    res = {"what": "evaluation loop, frames per second (pageable numpy in, metrics out), four variants alternated in one process",
           "shape": [H, W, D], "hint_density": p, "frames_per_window": n_frames, "rounds": rounds,
           "batch": next(iter(streams.values())).batch, "depth": next(iter(streams.values())).depth, "fps": {k: [] for k in streams}}
    try:
        for name in streams:               # warm-up: workspace, ring, first touch of everything
            run(name, streams[name].batch * 4)
        for tp in split.values():
            tp[0] = tp[1] = 0.0
        for _ in range(rounds):
            for name in streams:
                t0 = time.perf_counter()
                run(name, n_frames)
                res["fps"][name].append(round(n_frames / (time.perf_counter() - t0), 1))
        res["host_ms_per_frame"] = {k: {"push": round(tp[0] / (rounds * n_frames) * 1e3, 4), "pop": round(tp[1] / (rounds * n_frames) * 1e3, 4)}
                                    for k, tp in split.items()}
        res["reruns"] = {k: s.counts()[3] for k, s in streams.items()}
    finally:
        for s in streams.values():
            s.close()
    res["fps_median"] = {k: statistics.median(v) for k, v in res["fps"].items()}
    res["ms_per_frame_median"] = {k: round(1e3 / v, 4) for k, v in res["fps_median"].items()}
    f = res["fps"]
    if only is not None:
        print(json.dumps(res), flush=True)
        return
    res["device_over_plain_per_round"] = [round(b / d, 4) for b, d in zip(f["device_metrics"], f["plain"])]
    res["device_over_host_per_round"] = [round(b / a, 3) for b, a in zip(f["device_metrics"], f["host_metrics"])]
    res["only_over_plain_per_round"] = [round(c / d, 4) for c, d in zip(f["metrics_only"], f["plain"])]
    res["device_over_plain_median"] = statistics.median(res["device_over_plain_per_round"])
    print(json.dumps(res), flush=True)
    path = [a for a in sys.argv[1:] if a.endswith(".json")]
    if path:
        json.dump(res, open(path[0], "w"), indent=1)


if __name__ == "__main__":
    main()
