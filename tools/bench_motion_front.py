"""Times of the motion encoder's front (motion_kernels.hip) against what it replaces, at RAFT-Stereo's size for a
544x960 pair: maps of 136x240 with W3 = 240, 4 levels of radius 4, convc1 36 -> 64 (1x1) and convf1 2 -> 64 (7x7), B = 1, 4
and 8, float32 and bfloat16 pyramids, float32 and bfloat16 outputs.

  fused         one call of Engine.raft_motion_front: (cor1, flo1), the tensor of taps never written
  composition   Engine.raft_corr_lookup, then F.relu(F.conv2d(.)) for convc1 and for convf1, as BasicMotionEncoder.forward
                composes them (update.py:80,82); for bfloat16 outputs the lookup's float32 result and the flow are cast
                to bfloat16 first and the convolutions run in bfloat16, as they do under autocast
  lookup_alone  the lookup call by itself, for scale: it writes 36 channels where the fused call writes 128

The variants are alternated round by round in one process, so that a change of the machine's state falls on all of
them; every round times `--iters` calls between two device events after a warm-up.  Median, minimum and maximum over the
rounds are reported, with the bytes each side moves at the least (every tensor read or written once per launch that
touches it).  A speed-up counts only where the fused median is below the composition's by more than the larger of the
two ranges (max - min).  Writes one JSON document to --out and prints it."""
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


def row(stat, nbytes, launches):
    med, lo, hi = stat
    return dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), ms_range=round(hi - lo, 4), launches=launches,
                MB_moved=round(nbytes / 1e6, 2), GBps=round(nbytes / med / 1e6, 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_front.json"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds: at least five")
    eng = Engine()
    dev = eng.device
    H4, W2, W3, L, R, Cc, Cf, ks = 136, 240, 240, 4, 4, 64, 64, 7
    taps, K = 2 * R + 1, L * (2 * R + 1)
    out = {"shape": ["B", "C", H4, W2], "W3": W3, "levels": L, "radius": R, "convc1": [Cc, K, 1, 1], "convf1": [Cf, 2, ks, ks],
           "rounds": args.rounds, "iters_per_round": args.iters, "cases": {}}
    g = torch.Generator(device="cpu").manual_seed(7)
    wc = (torch.randn((Cc, K, 1, 1), generator=g) / K ** 0.5).to(dev)
    wf = (torch.randn((Cf, 2, ks, ks), generator=g) / (2 * ks * ks) ** 0.5).to(dev)
    bc, bf = (torch.randn(Cc, generator=g) * 0.5).to(dev), (torch.randn(Cf, generator=g) * 0.5).to(dev)
    wc16, wf16, bc16, bf16 = (t.bfloat16() for t in (wc, wf, bc, bf))
    for B in args.batches:
        N = B * H4 * W2
        # coordinates as the first iterations see them: the pixel's own column less a disparity, some left of the row
        xs = torch.arange(W2, dtype=torch.float32).view(1, 1, 1, W2).expand(B, 1, H4, W2)
        coords = torch.cat([xs - torch.rand((B, 1, H4, W2), generator=g) * 48, torch.zeros(B, 1, H4, W2)], dim=1).contiguous().to(dev)
        flow = torch.cat([coords[:, :1].cpu() - xs, torch.zeros(B, 1, H4, W2)], dim=1).contiguous().to(dev)
        base = torch.randn((B, H4, W2, 1, W3), generator=g).to(dev)
        for pname, pdtype, psize in (("float32", torch.float32, 4), ("bfloat16", torch.bfloat16, 2)):
            pyr = eng.raft_corr_pyramid(base.to(pdtype), None, None, L)
            look = torch.empty((B, K, H4, W2), dtype=torch.float32, device=dev)
            for oname, odtype, osize in (("float32", torch.float32, 4), ("bfloat16", torch.bfloat16, 2)):
                both = torch.empty((B, Cc + Cf, H4, W2), dtype=odtype, device=dev)
                halves = (both[:, :Cc], both[:, Cc:])

                def fused():
                    return eng.raft_motion_front(pyr, coords, flow, wc, bc, wf, bf, R, out=halves)

                if odtype == torch.float32:
                    def composition():
                        corr = eng.raft_corr_lookup(pyr, coords, R, out=look)
                        return F.relu(F.conv2d(corr, wc, bc)), F.relu(F.conv2d(flow, wf, bf, padding=ks // 2))
                    launches = 5
                else:
                    def composition():
                        corr = eng.raft_corr_lookup(pyr, coords, R, out=look)
                        return (F.relu(F.conv2d(corr.bfloat16(), wc16, bc16)), F.relu(F.conv2d(flow.bfloat16(), wf16, bf16, padding=ks // 2)))
                    launches = 7

                def lookup_alone():
                    return eng.raft_corr_lookup(pyr, coords, R, out=look)

                st = alternate({"fused": fused, "composition": composition, "lookup_alone": lookup_alone}, args.rounds, args.iters, warm_iters=5,
                               warm=5, round_warm=3)
                # per pixel and level the 128-byte lines the 2r+2 cells lie in (one or two), and the coordinate
                window = sum(min((taps + 1) * psize + 64, (W3 >> i) * psize) for i in range(L)) + 4
                chunks = (N + 127) // 128
                weights = (K * Cc + 2 * ks * ks * Cf + Cc + Cf) * 4
                b_fused = N * (window + 2 * 4 + (Cc + Cf) * osize) + min(chunks, 1024) * weights
                b_look = N * (window + K * 4)
                cast = 0 if odtype == torch.float32 else N * (K * (4 + 2) + 2 * (4 + 2))
                isize = osize                                             # what the convolutions read
                b_comp = b_look + cast + N * (K * isize + Cc * osize + 2 * Cc * osize + 2 * isize + Cf * osize + 2 * Cf * osize)
                case = {"fused": row(st["fused"], b_fused, 1), "composition": row(st["composition"], b_comp, launches),
                        "lookup_alone": row(st["lookup_alone"], b_look, 1)}
                f, c = case["fused"], case["composition"]
                case["composition_over_fused"] = round(c["ms"] / f["ms"], 2)
                case["fused_is_faster_beyond_the_ranges"] = bool(c["ms"] - f["ms"] > max(f["ms_range"], c["ms_range"]))
                a, b = fused(), composition()
                torch.cuda.synchronize()
                case["max_abs_diff_vs_composition"] = [float((x.float() - y.float()).abs().max().item()) for x, y in zip(a, b)]
                out["cases"][f"B{B}_pyramid_{pname}_out_{oname}"] = case
                del both, halves
            del pyr, look
        del base
        torch.cuda.empty_cache()
    out["fused_is_faster_at_every_B"] = all(c["fused_is_faster_beyond_the_ranges"] for c in out["cases"].values())
    out["device"] = eng.ctx.device_name
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
