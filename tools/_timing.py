"""Device-event timing the bench_*.py tools share."""
import statistics

import torch


def timeit(fn, iters, warm):
    """ms per call of fn over `iters` calls, after `warm` calls that are not timed."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, rounds, iters, warm_iters, warm, round_warm=1):
    """variants: name -> callable.  Every variant is first run once through timeit(fn, warm_iters, warm); then every round
    times each of them in turn (`iters` calls, or iters[name], after round_warm calls), so that a change of the machine's
    state falls on all of them; -> name -> (median ms, min ms, max ms) over the rounds."""
    for fn in variants.values():
        timeit(fn, warm_iters, warm)
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timeit(fn, iters[k] if isinstance(iters, dict) else iters, round_warm))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}
