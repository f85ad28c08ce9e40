#!/usr/bin/env python3
"""tools/viz_bench.py [out.json] [--rounds R] [--iters N] [--B B] [--H H --W W] [--dilation D]: milliseconds per frame of the
pictures test.py --outdir renders (utils.py:17-79, test.py:318-343) at 540x960, on the host and on the device, alternated round
after round in one process on one box:
  host    tests/_viz_ref.py, the numpy restatement of utils.py the tests hold to the reference's output (with its dilation, which
          the reference gets from OpenCV): guided_visualize (all six maps) and color_error_image_kitti, one frame per call,
          host clock
  dropin  vppstereo_amd.utils (numpy in, numpy out through the _host calls: upload, kernel, download), one frame per call,
          host clock
  device  Engine.guided_visualize (six maps, and 'avgerr' alone), Engine.error_colors, Engine.finite_max + Engine.colorize on
          resident tensors of B frames, device events around N calls after warm-up
No speed is promised anywhere; the ratios printed are what this run measured."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def main():
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    rounds, iters, B = arg("--rounds", 5), arg("--iters", 50), arg("--B", 8)
    H, W, d = arg("--height", 540), arg("--width", 960), arg("--dilation", 7)
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    import torch
    import _viz_ref as VR
    from vppstereo_amd import utils as U
    from vppstereo_amd.engine import Engine
    eng = Engine()        # raises without a device: there is nothing to measure then
    rng = np.random.default_rng(1)
    gt = rng.uniform(1, 190, (B, H, W)).astype(np.float32)
    err = np.where(rng.random((B, H, W)) < 0.7, rng.normal(0, 0.6, (B, H, W)), rng.uniform(-40, 40, (B, H, W)))
    disp = (gt + err).astype(np.float32)
    valid = (rng.random((B, H, W)) < 0.85).astype(np.float32)
    error = np.abs(disp - gt)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    t = lambda a: torch.from_numpy(a).to(eng.device)
    td, tg, tv, te, tl = t(disp), t(gt), t(valid), t(error), t(lut)
    out6 = torch.empty((6, B, H, W, 3), dtype=torch.uint8, device=eng.device)
    out1 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=eng.device)

    def host_clock(fn, n):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) * 1e3 / n          # one frame per call

    def device_events(fn):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters / B                   # B frames per call

    legs = {
        "host_guided_visualize": lambda: host_clock(lambda: VR.guided_visualize(disp[0], gt[0], valid[0], 1, d), 2),
        "host_error_colors": lambda: host_clock(lambda: VR.error_colors(error[0], 1, valid[0], True, d), 4),
        "dropin_guided_visualize": lambda: host_clock(lambda: U.guided_visualize(disp[0], gt[0], valid[0], dilation=d), 10),
        "dropin_error_colors": lambda: host_clock(lambda: U.color_error_image_kitti(error[0], mask=valid[0], dilation=d), 10),
        "device_guided_visualize": lambda: device_events(lambda: eng.guided_visualize(td, tg, tv, dilation=d, out=out6)),
        "device_guided_visualize_avgerr": lambda: device_events(lambda: eng.guided_visualize(td, tg, tv, dilation=d, which="avgerr", out=out6)),
        "device_guided_visualize_undilated": lambda: device_events(lambda: eng.guided_visualize(td, tg, tv, dilation=1, out=out6)),
        "device_error_colors": lambda: device_events(lambda: eng.error_colors(te, tv, dilation=d, out=out1)),
        "device_finite_max_colorize": lambda: device_events(lambda: eng.colorize(td, eng.finite_max(tg), tl, dilation=d, out=out1)),
    }
    # the legs compute the same pictures (checked once, outside the timed windows)
    want = VR.guided_visualize(disp[0], gt[0], valid[0], 1, d)
    got = eng.guided_visualize(td, tg, tv, dilation=d, out=out6)
    torch.cuda.synchronize()
    assert all(np.array_equal(got[k][0].cpu().numpy(), want[k]) for k in want)
    for name in legs:
        if not name.startswith("host_"):
            legs[name]()                                        # warm-up: workspace, code objects
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for name, leg in legs.items():                          # the legs take turns, round after round
            ms[name].append(leg())
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"what": "pictures of test.py --outdir, milliseconds per frame; host numpy (tests/_viz_ref.py), the numpy drop-in through the "
                   "_host calls, and the device calls on resident tensors, alternated in one process",
           "shape": [H, W], "dilation": d, "device_batch": B, "device_calls_per_window": iters, "rounds": rounds,
           "device": eng.ctx.device_name, "ms_per_frame": ms, "median_ms_per_frame": med,
           "ratio_host_over_device": {"guided_visualize": med["host_guided_visualize"] / med["device_guided_visualize"],
                                      "error_colors": med["host_error_colors"] / med["device_error_colors"]},
           "ratio_host_over_dropin": {"guided_visualize": med["host_guided_visualize"] / med["dropin_guided_visualize"],
                                      "error_colors": med["host_error_colors"] / med["dropin_error_colors"]}}
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
