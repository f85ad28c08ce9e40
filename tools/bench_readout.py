"""Times of the read-out kernels (readout_kernels.hip) against what they replace, at the size of a 544x960 pair:

  psmnet   Engine.psmnet_disparity on cost3 [B,1,48,136,240] -> [B,540,960] (maxdisp 192, the crop of test.py:242-245)
           against  models/psmnet/psmnet.py:227-233 + submodule.py:125-128 + the crop written out in torch on the same
           device: trilinear upsample to [B,1,192,544,960], squeeze, softmax, times the disparities, sum, slice
  raft     Engine.raft_upsample on flow [B,2,136,240] + mask [B,144,136,240] with channels=1, negate and the same crop
           against  RAFTStereo.upsample_flow (raft_stereo.py:69-81) + [:, :1] + the negation + the slice in torch

float32 and bfloat16, B = 1, 4 and 8.  The variants of one comparison are alternated round by round, so that a change
of the machine's state falls on both; median, minimum and maximum over the rounds are reported, with the bytes each
fused call has to move (input read once, output written once) and the rate that implies.  The torch side of PSMNet
allocates the upsampled volume (401 MB per frame in float32) and at least two more of its size; a batch it cannot hold
is reported as such and not timed.  Prints one JSON line and writes it to profiles/readout.json with --write."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vppstereo_amd.engine import Engine  # noqa: E402
from tools._timing import alternate  # noqa: E402


def row(stat, nbytes=None):
    med, lo, hi = stat
    r = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
    if nbytes is not None:
        r.update(MB_moved=round(nbytes / 1e6, 2), GBps=round(nbytes / med / 1e6, 1))
    return r


def torch_psm(cost3, maxdisp, size, crop):
    """psmnet.py:227-233, submodule.py:125-128, test.py:242-245."""
    c = F.interpolate(cost3, size=[maxdisp, size[0], size[1]], mode="trilinear", align_corners=False)
    pred = F.softmax(torch.squeeze(c, 1), dim=1)
    disp = torch.arange(maxdisp, dtype=pred.dtype, device=pred.device).view(1, maxdisp, 1, 1)
    out = torch.sum(pred * disp.repeat(pred.shape[0], 1, pred.shape[2], pred.shape[3]), 1)
    ht, wd = out.shape[-2:]
    return out[..., crop[2]:ht - crop[3], crop[0]:wd - crop[1]]


def torch_raft(flow, mask, n_downsample, crop):
    """raft_stereo.py:69-81, :154, test.py:238, :242-245."""
    N, D, H, W = flow.shape
    factor = 2 ** n_downsample
    m = torch.softmax(mask.view(N, 1, 9, factor, factor, H, W), dim=2)
    up = F.unfold(factor * flow, [3, 3], padding=1).view(N, D, 9, 1, 1, H, W)
    up = torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, D, factor * H, factor * W)
    pred = -up[:, :1].squeeze(1)
    ht, wd = pred.shape[-2:]
    return pred[..., crop[2]:ht - crop[3], crop[0]:wd - crop[1]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--write", action="store_true", help="also write profiles/readout.json")
    args = ap.parse_args()
    eng = Engine()
    dev = eng.device
    D4, H4, W4, D, H, W = 48, 136, 240, 192, 544, 960
    crop = [0, 0, 2, 2]                    # test.py's _pad for a 540x960 frame: [left, right, top, bottom]
    Ho, Wo = H - crop[2] - crop[3], W - crop[0] - crop[1]
    out = {"psmnet_shape": ["B", 1, D4, H4, W4], "maxdisp": D, "size": [H, W], "crop": crop, "raft_shape": [["B", 2, H4, W4], ["B", 144, H4, W4]],
           "rounds": args.rounds, "iters_per_round": args.iters, "cases": {}}
    g = torch.Generator(device="cpu").manual_seed(7)
    for B in args.batches:
        cost32 = (torch.randn((B, 1, D4, H4, W4), generator=g) * 3).to(dev)
        flow32 = (torch.randn((B, 2, H4, W4), generator=g) * 12).to(dev)
        mask32 = (torch.randn((B, 144, H4, W4), generator=g) * 2.5).to(dev)
        for name, dtype, size in (("float32", torch.float32, 4), ("bfloat16", torch.bfloat16, 2)):
            case = {}
            cost, flow, mask = cost32.to(dtype), flow32.to(dtype), mask32.to(dtype)
            res = torch.empty((B, Ho, Wo), dtype=torch.float32, device=dev)
            variants = {"fused": lambda: eng.psmnet_disparity(cost, D, (H, W), crop=crop, out=res)}
            iters = {"fused": args.iters, "torch_composition": max(1, args.iters // 5)}
            try:
                torch_psm(cost, D, (H, W), crop)
                torch.cuda.synchronize()
                variants["torch_composition"] = lambda: torch_psm(cost, D, (H, W), crop)
            except torch.OutOfMemoryError:
                case["psmnet_torch_composition"] = "out of memory"
            torch.cuda.empty_cache()
            st = alternate(variants, args.rounds, iters, warm_iters=1, warm=1)
            case["psmnet_fused"] = row(st["fused"], cost.numel() * size + res.numel() * 4)
            if "torch_composition" in st:
                case["psmnet_torch_composition"] = row(st["torch_composition"])
                case["psmnet_speedup"] = round(st["torch_composition"][0] / st["fused"][0], 2)
                if dtype == torch.float32:
                    d = (eng.psmnet_disparity(cost, D, (H, W), crop=crop) - torch_psm(cost, D, (H, W), crop)).abs().max()
                    case["psmnet_max_abs_diff_vs_torch_px"] = float(d.item())
            torch.cuda.empty_cache()

            up = torch.empty((B, 1, Ho, Wo), dtype=torch.float32, device=dev)
            variants = {"fused": lambda: eng.raft_upsample(flow, mask, 2, negate=True, channels=1, crop=crop, out=up),
                        "torch_composition": lambda: torch_raft(flow, mask, 2, crop)}
            st = alternate(variants, args.rounds, {"fused": args.iters, "torch_composition": args.iters}, warm_iters=1, warm=1)
            case["raft_fused"] = row(st["fused"], (mask.numel() + flow.numel() // 2) * size + up.numel() * 4)
            case["raft_torch_composition"] = row(st["torch_composition"])
            case["raft_speedup"] = round(st["torch_composition"][0] / st["fused"][0], 2)
            if dtype == torch.float32:
                d = (eng.raft_upsample(flow, mask, 2, negate=True, channels=1, crop=crop)[:, 0] - torch_raft(flow, mask, 2, crop)).abs().max()
                case["raft_max_abs_diff_vs_torch_px"] = float(d.item())
            out["cases"][f"B{B}_{name}"] = case
            del cost, flow, mask, res, up
            torch.cuda.empty_cache()
        del cost32, flow32, mask32
    out["device"] = eng.ctx.device_name
    line = json.dumps(out)
    print(line)
    if args.write:
        with open(os.path.join(ROOT, "profiles", "readout.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
