"""Times of the fused correlation call (corr_gemm_kernels.hip: GEMM on the matrix cores, / sqrt(D), hint modulation and
pyramid in one launch) against what it replaces, at RAFT-Stereo's size for a 544x960 pair: feature maps [B,256,136,240],
B = 1, 4 and 8, float32 and bfloat16, with hints.

  fused          Engine.raft_corr_fused
  block          today's block: Engine.raft_corr (torch's einsum and division) followed by Engine.raft_corr_pyramid with
                 hints
  einsum         float32 only: torch's einsum alone, which is what the GEMM by itself costs there

The variants are alternated round by round, so that a change of the machine's state falls on all of them; median,
minimum and maximum over the rounds are reported, with the bytes each moves at the least (every tensor read or written
once) and the rate that implies, and for the fused call the matrix rate its time implies.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vppstereo_amd.engine import Engine  # noqa: E402
from tools._timing import alternate  # noqa: E402


def row(stat, nbytes, flop=None):
    med, lo, hi = stat
    r = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), MB_moved=round(nbytes / 1e6, 2),
             GBps=round(nbytes / med / 1e6, 1))
    if flop is not None:
        r["TFLOPs"] = round(flop / med / 1e9, 1)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    eng = Engine()
    dev = eng.device
    D, H4, W2, W3, H, W, L = 256, 136, 240, 240, 544, 960, 4
    out = {"features": ["B", D, H4, W2], "levels": L, "rounds": args.rounds, "iters_per_round": args.iters, "cases": {}}
    g = torch.Generator(device="cpu").manual_seed(5)
    for B in args.batches:
        N = B * H4 * W2
        valid = (torch.rand((B, 1, H, W), generator=g) < 0.03).float().to(dev)
        hints = (torch.rand((B, 1, H, W), generator=g) * 190 + 1).to(dev) * valid
        rows = int((F.interpolate(valid, size=[H4, W2], mode="nearest") != 0).sum().item())
        b2, b3 = torch.randn((B, D, H4, W2), generator=g).to(dev), torch.randn((B, D, H4, W3), generator=g).to(dev)
        for name, dtype, size in (("float32", torch.float32, 4), ("bfloat16", torch.bfloat16, 2)):
            f2, f3 = b2.to(dtype), b3.to(dtype)
            variants = {"fused": lambda: eng.raft_corr_fused(f2, f3, hints, valid, L),
                        "block": lambda: eng.raft_corr_pyramid(eng.raft_corr(f2, f3), hints, valid, L)}
            if dtype == torch.float32:
                variants["einsum"] = lambda: torch.einsum('aijk,aijh->ajkh', f2, f3)
            st = alternate(variants, args.rounds, args.iters, warm_iters=2, warm=2)
            feat = (f2.numel() + f3.numel()) * size
            vol = N * W3 * size
            pooled = sum(N * (W3 >> i) for i in range(1, L)) * size
            flop = 2.0 * D * N * W3
            case = {"rows_with_a_hint": rows, "rows": N}
            # fused: the two feature maps in, level 0 and levels 1..3 out
            case["fused"] = row(st["fused"], feat + vol + pooled, flop)
            # block: the GEMM (features in, volume out), the division (volume in and out), the pyramid pass (volume in,
            # hinted rows out, levels 1..3 out)
            case["block"] = row(st["block"], feat + vol + 2 * vol + vol + rows * W3 * size + pooled)
            case["speedup"] = round(st["block"][0] / st["fused"][0], 2)
            if "einsum" in st:
                case["einsum"] = row(st["einsum"], feat + vol, flop)
            out["cases"][f"B{B}_{name}"] = case
            del f2, f3
        del b2, b3
        torch.cuda.empty_cache()
    out["device"] = eng.ctx.device_name
    print(json.dumps(out))


if __name__ == "__main__":
    main()
