"""Times of the correlation pyramid and lookup (corr_kernels.hip) against what they replace, at RAFT-Stereo's size for
a 544x960 pair: the volume [B,136,240,1,240], B = 1, 4 and 8, float32 and bfloat16.

  pyramid   the fused call with hints (modulation + three pooled levels, one pass)  against
            vppx_raft_corr_modulate_dt_dev followed by torch's avg_pool2d, as CorrBlock1D.__init__ composes them
            (four of them: the reference pools once more than it reads)
  lookup    one call of the kernel (4 levels, radius 4)  against  CorrBlock1D.__call__ written out in torch on the
            same device: linspace, add, divide, cat, normalise, grid_sample per level, then cat, permute, copy

The variants of one comparison are alternated round by round, so that a change of the machine's state falls on all of
them; median, minimum and maximum over the rounds are reported, with the bytes each call moves at the least (every
tensor read or written once) and the rate that implies.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vppstereo_amd.engine import Engine  # noqa: E402
from tools._timing import alternate  # noqa: E402


def row(stat, nbytes):
    med, lo, hi = stat
    return dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), MB_moved=round(nbytes / 1e6, 2),
                GBps=round(nbytes / med / 1e6, 1))


def torch_lookup(pyramid, coords, radius):
    """CorrBlock1D.__call__ (models/raft_stereo/corr.py:126-145) on tensors [N,1,1,Wi]."""
    r = radius
    coords = coords[:, :1].permute(0, 2, 3, 1)
    batch, h1, w1, _ = coords.shape
    levels = []
    for i, corr in enumerate(pyramid):
        dx = torch.linspace(-r, r, 2 * r + 1).view(1, 1, 2 * r + 1, 1).to(coords.device)
        x0 = dx + coords.reshape(batch * h1 * w1, 1, 1, 1) / 2 ** i
        y0 = torch.zeros_like(x0)
        W = corr.shape[-1]
        grid = torch.cat([2 * x0 / (W - 1) - 1, y0], dim=-1).to(corr.dtype)      # grid_sample wants the volume's dtype
        levels.append(F.grid_sample(corr, grid, align_corners=True).view(batch, h1, w1, -1))
    return torch.cat(levels, dim=-1).permute(0, 3, 1, 2).contiguous().float()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    eng = Engine()
    dev = eng.device
    H4, W2, W3, H, W, L, R = 136, 240, 240, 544, 960, 4, 4
    taps = 2 * R + 1
    out = {"shape": ["B", H4, W2, 1, W3], "levels": L, "radius": R, "rounds": args.rounds, "iters_per_round": args.iters, "cases": {}}
    g = torch.Generator(device="cpu").manual_seed(5)
    for B in args.batches:
        N = B * H4 * W2
        valid = (torch.rand((B, 1, H, W), generator=g) < 0.03).float().to(dev)
        hints = (torch.rand((B, 1, H, W), generator=g) * 190 + 1).to(dev) * valid
        rows = int((F.interpolate(valid, size=[H4, W2], mode="nearest") != 0).sum().item())
        # coordinates as the first iterations see them: the pixel's own column less a disparity, some left of the row
        xs = torch.arange(W2, dtype=torch.float32).view(1, 1, 1, W2).expand(B, 1, H4, W2)
        coords = torch.cat([xs - torch.rand((B, 1, H4, W2), generator=g) * 48, torch.zeros(B, 1, H4, W2)], dim=1).contiguous().to(dev)
        base = torch.randn((B, H4, W2, 1, W3), generator=g).to(dev)
        for name, dtype, size in (("float32", torch.float32, 4), ("bfloat16", torch.bfloat16, 2)):
            corr = base.to(dtype)
            work = corr.clone()
            pooled = sum(N * (W3 >> i) for i in range(1, L))

            # in place and repeated: the values change from call to call, the work does not depend on them
            def fused():
                return eng.raft_corr_pyramid(work, hints, valid, L)

            def separate():
                eng.raft_corr_modulate_(work, hints, valid)
                lv = work.view(N, 1, 1, W3)
                pyr = [lv]
                for _ in range(L):
                    lv = F.avg_pool2d(lv, [1, 2], stride=[1, 2])
                    pyr.append(lv)
                return pyr
            st = alternate({"fused": fused, "modulate_then_avg_pool2d": separate}, args.rounds, args.iters, warm_iters=2, warm=2)
            vol = N * W3 * size
            case = {"rows_with_a_hint": rows, "rows": N}
            # fused: level 0 read once, hinted rows written back, levels 1..3 written
            case["pyramid_fused"] = row(st["fused"], vol + rows * W3 * size + pooled * size)
            # separate: the modulation reads and writes the hinted rows; each pooling reads a level and writes the next (four)
            sep = 2 * rows * W3 * size + sum((N * (W3 >> i) + N * (W3 >> (i + 1))) * size for i in range(L))
            case["pyramid_modulate_then_avg_pool2d"] = row(st["modulate_then_avg_pool2d"], sep)
            case["pyramid_speedup"] = round(st["modulate_then_avg_pool2d"][0] / st["fused"][0], 2)

            work.copy_(corr)
            pyr = eng.raft_corr_pyramid(work, hints, valid, L)
            res = torch.empty((B, L * taps, H4, W2), dtype=torch.float32, device=dev)
            variants = {"kernel": lambda: eng.raft_corr_lookup(pyr, coords, R, out=res)}
            variants["torch_composition"] = lambda: torch_lookup(pyr, coords, R)
            st = alternate(variants, args.rounds, args.iters, warm_iters=2, warm=2)
            # what one lookup has to move: per pixel and level the 128-byte lines its 2r+2 cells lie in (one or two),
            # the coordinate, and the float32 result
            window = sum(min((taps + 1) * size + 64, (W3 >> i) * size) for i in range(L))
            moved = N * (window + 4 + L * taps * 4)
            case["lookup_kernel"] = row(st["kernel"], moved)
            case["lookup_torch_composition"] = row(st["torch_composition"], moved)
            case["lookup_speedup"] = round(st["torch_composition"][0] / st["kernel"][0], 2)
            if dtype == torch.float32:
                a, b = eng.raft_corr_lookup(pyr, coords, R), torch_lookup(pyr, coords, R)
                case["lookup_cells_unequal_to_torch"] = int((a.view(torch.int32) != b.view(torch.int32)).sum().item())
                case["lookup_max_abs_diff_vs_torch"] = float((a - b).abs().max().item())
            out["cases"][f"B{B}_{name}"] = case
            del corr, work, pyr, res
        del base
        torch.cuda.empty_cache()
    out["device"] = eng.ctx.device_name
    print(json.dumps(out))


if __name__ == "__main__":
    main()
