"""Time of one update iteration's glue (gru_kernels.hip through vppstereo_amd.update) against the reference's lines
written out in torch on the same device, at the size of a 544x960 pair:

  net   [B,128,136,240], [B,128,68,120], [B,128,34,60];  the context's [cz|cr|cq] per level as the three channel slices
        of one [B,384,h,w] tensor (raft_stereo.py:104);  the encoder's output [B,126,136,240] and flow [B,2,136,240]

  fused   GruGlue.fused_gru three times, in BasicMultiUpdateBlock.forward's order (update.py:121-133): per GRU one
          raft_gru_assemble into the kept hx buffer, one raft_gru_reset over it and one raft_gru_update: 9 launches
  torch   update.py:23-32, :87, :89-90, :95-97 as the reference has them: pool2x, interp, the cats, sigmoid(conv + c)
          twice, r * h, the third cat, tanh(conv + c), (1 - z) * h + z * q

On BOTH sides the nine gate convolutions and the encoder are stand-ins that return preallocated tensors, so that only the
glue is timed; what the glue hands them is computed and dropped.  float32 and bfloat16, B = 1, 4 and 8.  The two variants
are alternated round by round, so that a change of the machine's state falls on both; median, minimum and maximum over
the rounds are reported, with the bytes the fused launches have to move (every operand read once, every result written
once) and the rate that implies.  The times are device events around the whole Python loop and so include the host's
launch cost on both sides.  A frame runs 32 iterations (test.py's --iters): "per_frame_ms" is the iteration's time
multiplied by 32, not a measurement of its own.  Prints one JSON line and writes it to profiles/gru_glue.json with --write."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vppstereo_amd.engine import Engine  # noqa: E402
from tools._timing import alternate  # noqa: E402
from vppstereo_amd.update import GruGlue  # noqa: E402

ITERS_PER_FRAME = 32


def row(stat, nbytes=None):
    med, lo, hi = stat
    r = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), per_frame_ms=round(med * ITERS_PER_FRAME, 3))
    if nbytes is not None:
        r.update(MB_moved=round(nbytes / 1e6, 2), GBps=round(nbytes / med / 1e6, 1))
    return r


def pool2x(x):
    return F.avg_pool2d(x, 3, stride=2, padding=1)


def interp(x, dest):
    return F.interpolate(x, dest.shape[2:], mode="bilinear", align_corners=True)


def torch_gru(gru, h, cz, cr, cq, *x_list):
    """ConvGRU.forward (update.py:23-32)."""
    x = torch.cat(x_list, dim=1)
    hx = torch.cat([h, x], dim=1)
    z = torch.sigmoid(gru.convz(hx) + cz)
    r = torch.sigmoid(gru.convr(hx) + cr)
    q = torch.tanh(gru.convq(torch.cat([r * h, x], dim=1)) + cq)
    return (1 - z) * h + z * q


def torch_iteration(grus, net, inp, enc_out, flow):
    """BasicMultiUpdateBlock.forward (update.py:121-133) with the encoder's convolutions taken out: its cat (:87) stays."""
    n2 = torch_gru(grus[2], net[2], *inp[2], pool2x(net[1]))
    n1 = torch_gru(grus[1], net[1], *inp[1], pool2x(net[0]), interp(n2, net[1]))
    motion = torch.cat([enc_out, flow], dim=1)
    n0 = torch_gru(grus[0], net[0], *inp[0], motion, interp(n1, net[0]))
    return n0, n1, n2


def fused_iteration(glue, grus, net, inp, enc_out, flow):
    n2 = glue.fused_gru(grus[2], net[2], *inp[2], (net[1], "pool2x"), level=32)
    n1 = glue.fused_gru(grus[1], net[1], *inp[1], (net[0], "pool2x"), (n2, "interp"), level=16)
    n0 = glue.fused_gru(grus[0], net[0], *inp[0], enc_out, flow, (n1, "interp"), level=8)
    return n0, n1, n2


def fused_bytes(B, C, sizes, size):
    """Bytes the nine launches move: assemble reads its sources and writes hx; reset reads ar, cr, h and writes C
    channels; update reads az, cz, aq, cq, h and writes C channels."""
    px = [h * w for h, w in sizes]
    asm = [(C * px[0] + 126 * px[0] + 2 * px[0] + C * px[1]) + (2 * C + 128) * px[0],      # gru08: h, enc, flow, net1 -> hx08
           (C * px[1] + C * px[0] + C * px[2]) + 3 * C * px[1],                             # gru16: h, net0, net2 -> hx16
           (C * px[2] + C * px[1]) + 2 * C * px[2]]                                         # gru32: h, net1 -> hx32
    gates = sum((4 + 6) * C * p for p in px)
    return B * size * (sum(asm) + gates)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--write", action="store_true", help="also write profiles/gru_glue.json")
    args = ap.parse_args()
    eng = Engine()
    dev = eng.device
    C, sizes = 128, [(136, 240), (68, 120), (34, 60)]
    out = {"net_shapes": [["B", C, h, w] for h, w in sizes], "iterations_per_frame": ITERS_PER_FRAME, "rounds": args.rounds,
           "iters_per_round": args.iters, "fused_launches_per_iteration": 9, "cases": {}}
    g = torch.Generator(device="cpu").manual_seed(11)
    for B in args.batches:
        for name, dtype, size in (("float32", torch.float32, 4), ("bfloat16", torch.bfloat16, 2)):
            rnd = lambda *s, scale=1.0: (torch.randn(s, generator=g) * scale).to(dev).to(dtype)      # noqa: E731
            net = [torch.tanh(rnd(B, C, h, w)) for h, w in sizes]
            inp = [list(rnd(B, 3 * C, h, w, scale=2.0).split(C, dim=1)) for h, w in sizes]
            enc_out, flow = torch.relu(rnd(B, 126, *sizes[0])), rnd(B, 2, *sizes[0], scale=3.0)
            grus = []
            for h, w in sizes:          # the stand-ins: what a convolution would return, made once
                az, ar, aq = (rnd(B, C, h, w, scale=2.0) for _ in range(3))
                grus.append(SimpleNamespace(convz=lambda hx, t=az: t, convr=lambda hx, t=ar: t, convq=lambda hx, t=aq: t))
            glue = GruGlue()
            variants = {"fused": lambda: fused_iteration(glue, grus, net, inp, enc_out, flow),
                        "torch_composition": lambda: torch_iteration(grus, net, inp, enc_out, flow)}
            with torch.no_grad():
                st = alternate(variants, args.rounds, args.iters, warm_iters=2, warm=2)
                a, b = fused_iteration(glue, grus, net, inp, enc_out, flow), torch_iteration(grus, net, inp, enc_out, flow)
            case = {"fused": row(st["fused"], fused_bytes(B, C, sizes, size)), "torch_composition": row(st["torch_composition"]),
                    "torch_over_fused": round(st["torch_composition"][0] / st["fused"][0], 2),
                    "max_abs_diff_vs_torch": [float((x.float() - y.float()).abs().max().item()) for x, y in zip(a, b)]}
            out["cases"][f"B{B}_{name}"] = case
            del net, inp, enc_out, flow, grus, glue, a, b
            torch.cuda.empty_cache()
    out["device"] = eng.ctx.device_name
    print(json.dumps(out))
    if args.write:
        with open(os.path.join(ROOT, "profiles", "gru_glue.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
