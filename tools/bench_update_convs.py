"""Time of the update block's other convolutions on the library's kernel (FusedUpdate(block, convs=True): seven launches of
Engine.raft_conv) against torch's, at gru08's level of a 544x960 pair, on a block with the reference's channel counts.  --downs
says what that level is: 8 is 1/8 of the frame (68 x 120, the levels below 34 x 60 and 17 x 30), 4 is what tools/bench_gru_conv.py
takes, gru08 at 1/4 of the frame as n_downsample = 2 makes it (136 x 240, 68 x 120, 34 x 60).  Both by default.

  encoder   convc1 1x1 36 -> 64, convc2 3x3 64 -> 64, convf1 7x7 2 -> 64, convf2 3x3 64 -> 64, conv 3x3 128 -> 126
  gru08 / gru16 / gru32   3x3, 384 / 384 / 256 -> 128
  flow_head 3x3 128 -> 256, ReLU, 3x3 256 -> 2;   mask 3x3 128 -> 256, ReLU, 1x1 256 -> 144, .25 *

  A   FusedUpdate(block, motion_front=True, gru_conv=True)
  B   the same with convs=True

The timed units: the motion tail (convc2, convf2 and conv on the front's two outputs; A: three convolutions, three ReLUs and a cat),
the flow head, the mask head with its `.25 *`, the whole iteration (forward with a deferred lookup), and the whole iteration with
mask=False on both sides.  float32 and bfloat16, B = 1 and 4.  A and B are alternated round by round, so that a change of the
machine's state falls on both; median, minimum and maximum over the rounds are reported.  The times are device events around the
whole Python loop and so include the host's launch cost on both sides.  "B_faster" / "A_faster" say whether the medians differ by
more than the larger of the two ranges.  Prints one JSON line and writes it to profiles/update_convs.json with --write."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vppstereo_amd.engine import Engine  # noqa: E402
from tools._timing import alternate  # noqa: E402
from vppstereo_amd.corr import CorrBlock1DFused  # noqa: E402
from vppstereo_amd.update import FusedUpdate  # noqa: E402

C, FEAT, LEVELS, RADIUS = 128, 256, 4, 4
FRAME = (544, 960)


def sizes_of(down):
    return [(FRAME[0] // (down << k), FRAME[1] // (down << k)) for k in range(3)]


def make_block(dtype, dev):
    nn = torch.nn
    conv = lambda cin, cout, k: nn.Conv2d(cin, cout, k, padding=k // 2)        # noqa: E731

    def gru(cin):
        g = nn.Module()
        g.convz, g.convr, g.convq = conv(cin, C, 3), conv(cin, C, 3), conv(cin, C, 3)
        return g

    blk = nn.Module()
    blk.n_gru_layers = 3
    enc = blk.encoder = nn.Module()
    enc.convc1, enc.convc2 = conv(LEVELS * (2 * RADIUS + 1), 64, 1), conv(64, 64, 3)
    enc.convf1, enc.convf2 = conv(2, 64, 7), conv(64, 64, 3)
    enc.conv = conv(128, 126, 3)
    blk.gru08, blk.gru16, blk.gru32 = gru(3 * C), gru(3 * C), gru(2 * C)
    blk.flow_head = nn.Sequential(conv(C, 256, 3), nn.ReLU(), conv(256, 2, 3))
    blk.mask = nn.Sequential(conv(C, 256, 3), nn.ReLU(), conv(256, 9 * 16, 1))
    for p in blk.parameters():
        p.requires_grad_(False)
    return blk.to(device=dev, dtype=dtype).eval()


def row(stat):
    med, lo, hi = stat
    return dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--downs", type=int, nargs="+", default=[8, 4], help="gru08's level as a fraction of the frame")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--write", action="store_true", help="also write profiles/update_convs.json")
    args = ap.parse_args()
    eng = Engine()
    dev = eng.device
    torch.manual_seed(17)
    macs = {"motion_tail": 9 * (64 * 64 * 2 + 128 * 126), "flow_head": 9 * (C * 256 + 256 * 2), "mask_head": 9 * C * 256 + 256 * 144}
    out = {"frame": list(FRAME), "net_shapes": {f"down{d}": [["B", C, h, w] for h, w in sizes_of(d)] for d in args.downs},
           "rounds": args.rounds, "iters_per_round": args.iters, "multiply_adds_per_pixel": macs, "cases": {}}
    g = torch.Generator(device="cpu").manual_seed(19)
    for down, B in [(d, b) for d in args.downs for b in args.batches]:
        SIZES = sizes_of(down)
        px = SIZES[0][0] * SIZES[0][1]
        for name, dtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
            rnd = lambda *s, scale=1.0: (torch.randn(s, generator=g) * scale).to(dev)      # noqa: E731
            blk = make_block(dtype, dev)
            fused = {"A": FusedUpdate(blk, motion_front=True, gru_conv=True), "B": FusedUpdate(blk, motion_front=True, gru_conv=True, convs=True)}
            net = [torch.tanh(rnd(B, C, h, w)).to(dtype) for h, w in SIZES]
            inp = [list(rnd(B, 3 * C, h, w).to(dtype).split(C, dim=1)) for h, w in SIZES]
            h8, w8 = SIZES[0]
            corr_fn = CorrBlock1DFused(rnd(B, FEAT, h8, w8, scale=0.25), rnd(B, FEAT, h8, w8, scale=0.25), radius=RADIUS, num_levels=LEVELS)
            xs = torch.arange(w8, dtype=torch.float32, device=dev).view(1, 1, 1, w8).expand(B, 1, h8, w8)
            ys = torch.arange(h8, dtype=torch.float32, device=dev).view(1, 1, h8, 1).expand(B, 1, h8, w8)
            flow32 = torch.cat([rnd(B, 1, h8, w8, scale=3.0), torch.zeros(B, 1, h8, w8, device=dev)], dim=1)
            coords = torch.cat([xs, ys], dim=1) + flow32
            flow = flow32.to(dtype)
            cor, flo = (t.to(dtype) for t in (torch.relu(rnd(B, 64, h8, w8)), torch.relu(rnd(B, 64, h8, w8))))

            def iteration(k, mask=True):
                return fused[k]([t for t in net], inp, corr_fn.deferred(coords), flow, mask=mask)

            units = {"motion_tail": lambda k: fused[k]._motion_tail(blk.encoder, cor, flo, dtype),
                     "flow_head": lambda k: fused[k]._head(blk.flow_head, net[0], dtype, "flow_head"),
                     "mask_head": lambda k: fused[k]._head(blk.mask, net[0], dtype, "mask", scale=.25),
                     "iteration": iteration, "iteration_without_mask": lambda k: iteration(k, mask=False)}
            case = {}
            with torch.no_grad():
                for unit, fn in units.items():
                    st = alternate({"A": lambda: fn("A"), "B": lambda: fn("B")}, args.rounds, args.iters, warm_iters=2, warm=2)
                    (a, alo, ahi), (b, blo, bhi) = st["A"], st["B"]
                    case[unit] = {"A": row(st["A"]), "B": row(st["B"]), "A_over_B": round(a / b, 3),
                                  "B_faster": bool(a - b > max(ahi - alo, bhi - blo)), "A_faster": bool(b - a > max(ahi - alo, bhi - blo))}
                    if unit in macs:
                        case[unit]["GFLOP"] = round(2 * macs[unit] * B * px / 1e9, 2)
                (na, ma, da), (nb, mb, db) = iteration("A"), iteration("B")
                case["max_abs_diff_A_vs_B"] = {"net0": float((na[0].float() - nb[0].float()).abs().max().item()),
                                               "mask": float((ma.float() - mb.float()).abs().max().item()),
                                               "delta_flow": float((da.float() - db.float()).abs().max().item())}
            out["cases"][f"down{down}_B{B}_{name}"] = case
            del blk, fused, net, inp, corr_fn, cor, flo, na, ma, da, nb, mb, db
            torch.cuda.empty_cache()
    out["device"] = eng.ctx.device_name
    print(json.dumps(out))
    if args.write:
        with open(os.path.join(ROOT, "profiles", "update_convs.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
