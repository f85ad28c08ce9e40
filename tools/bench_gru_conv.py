"""Time of a ConvGRU with its convolutions on the library's kernel (conv_kernels.hip through GruGlue.fused_gru(conv=True))
against the same GRU with torch's convolutions between the glue launches (fused_gru as it was), at the size of a 544x960 pair:

  net   [B,128,136,240], [B,128,68,120], [B,128,34,60];  the context's [cz|cr|cq] per level as the three channel slices
        of one [B,384,h,w] tensor;  the encoder's output [B,126,136,240] and flow [B,2,136,240]
  gru08 384 -> 128 channels, gru16 384 -> 128, gru32 256 -> 128: seeded nn.Conv2d(.., 3, padding=1) in the working dtype

  A   fused_gru(conv=False): raft_gru_assemble, convz, convr (torch), raft_gru_reset, convq (torch), raft_gru_update:
      6 launches per GRU, 18 per iteration
  B   fused_gru(conv=True):  raft_gru_assemble, raft_gru_zr, raft_gru_q: 3 launches per GRU, 9 per iteration

The timed units are one GRU per level and the three together in BasicMultiUpdateBlock.forward's order; the motion encoder,
flow_head and mask are not run on either side (the encoder's output is a preallocated tensor).  float32 and bfloat16, B = 1
and 4.  A and B are alternated round by round, so that a change of the machine's state falls on both; median, minimum and
maximum over the rounds are reported.  The times are device events around the whole Python loop and so include the host's
launch cost on both sides.  Next to each time: the FLOPs of the unit's convolutions (2 * 9 * Cin * Cout per pixel, counted)
and the rate they imply against the matrix cores' peak for the dtype (2500 TFLOP/s bfloat16, 157.3 TFLOP/s float32); the
assembly's time is inside the unit, so the rate is a lower bound of the kernel's.  "B_faster" says whether the medians differ
by more than the larger of the two ranges.  Prints one JSON line and writes it to profiles/gru_conv.json with --write."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vppstereo_amd.engine import Engine  # noqa: E402
from tools._timing import alternate  # noqa: E402
from vppstereo_amd.update import GruGlue  # noqa: E402

PEAK_TFLOPS = {"float32": 157.3, "bfloat16": 2500.0}
C, SIZES = 128, [(136, 240), (68, 120), (34, 60)]
CIN = {8: 384, 16: 384, 32: 256}


def row(stat, flops, peak):
    med, lo, hi = stat
    return dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), TFLOPs=round(flops / med / 1e9, 1),
                of_peak=round(flops / med / 1e9 / peak, 4))


def make_gru(cin, dtype, dev):
    g = SimpleNamespace(**{cv: torch.nn.Conv2d(cin, C, 3, padding=1) for cv in ("convz", "convr", "convq")})
    for m in vars(g).values():
        m.to(device=dev, dtype=dtype)
    return g


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--write", action="store_true", help="also write profiles/gru_conv.json")
    args = ap.parse_args()
    eng = Engine()
    dev = eng.device
    torch.manual_seed(13)
    out = {"net_shapes": [["B", C, h, w] for h, w in SIZES], "gru_channels_in": CIN, "rounds": args.rounds, "iters_per_round": args.iters,
           "launches_per_iteration": {"A": 18, "B": 9}, "peak_TFLOPs": PEAK_TFLOPS, "cases": {}}
    g = torch.Generator(device="cpu").manual_seed(11)
    for B in args.batches:
        for name, dtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
            rnd = lambda *s, scale=1.0: (torch.randn(s, generator=g) * scale).to(dev).to(dtype)      # noqa: E731
            net = [torch.tanh(rnd(B, C, h, w)) for h, w in SIZES]
            inp = [list(rnd(B, 3 * C, h, w).split(C, dim=1)) for h, w in SIZES]
            enc_out, flow = torch.relu(rnd(B, 126, *SIZES[0])), rnd(B, 2, *SIZES[0], scale=3.0)
            grus = {lvl: make_gru(CIN[lvl], dtype, dev) for lvl in (8, 16, 32)}
            glue = {False: GruGlue(), True: GruGlue()}

            def gru08(conv, n1=None):
                return glue[conv].fused_gru(grus[8], net[0], *inp[0], enc_out, flow, (net[1] if n1 is None else n1, "interp"), level=8, conv=conv)

            def gru16(conv, n2=None):
                return glue[conv].fused_gru(grus[16], net[1], *inp[1], (net[0], "pool2x"), (net[2] if n2 is None else n2, "interp"), level=16,
                                            conv=conv)

            def gru32(conv):
                return glue[conv].fused_gru(grus[32], net[2], *inp[2], (net[1], "pool2x"), level=32, conv=conv)

            def iteration(conv):
                n2 = gru32(conv)
                n1 = gru16(conv, n2)
                return gru08(conv, n1), n1, n2

            px = [B * h * w for h, w in SIZES]
            flops = {"gru08": 3 * 2 * 9 * CIN[8] * C * px[0], "gru16": 3 * 2 * 9 * CIN[16] * C * px[1], "gru32": 3 * 2 * 9 * CIN[32] * C * px[2]}
            flops["iteration"] = sum(flops.values())
            units = {"gru08": gru08, "gru16": gru16, "gru32": gru32, "iteration": iteration}
            case = {}
            with torch.no_grad():
                for unit, fn in units.items():
                    st = alternate({"A": lambda: fn(False), "B": lambda: fn(True)}, args.rounds, args.iters, warm_iters=2, warm=2)
                    (a, alo, ahi), (b, blo, bhi) = st["A"], st["B"]
                    case[unit] = {"GFLOP": round(flops[unit] / 1e9, 2), "A": row(st["A"], flops[unit], PEAK_TFLOPS[name]),
                                  "B": row(st["B"], flops[unit], PEAK_TFLOPS[name]), "A_over_B": round(a / b, 3),
                                  "B_faster": bool(a - b > max(ahi - alo, bhi - blo)), "A_faster": bool(b - a > max(ahi - alo, bhi - blo))}
                xa, xb = iteration(False), iteration(True)
                case["max_abs_diff_A_vs_B"] = [float((x.float() - y.float()).abs().max().item()) for x, y in zip(xa, xb)]
            out["cases"][f"B{B}_{name}"] = case
            del net, inp, enc_out, flow, grus, glue, xa, xb
            torch.cuda.empty_cache()
    out["device"] = eng.ctx.device_name
    print(json.dumps(out))
    if args.write:
        with open(os.path.join(ROOT, "profiles", "gru_conv.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
