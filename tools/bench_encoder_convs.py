"""Time of the two encoders' convolutions on the library's kernel (FusedEncoder(encoder, convs=True): every convolution but the
7x7 stem one launch of Engine.raft_conv, at stride 1 or 2) against torch's in the same wrapper, at the size of a 544x960 pair, on
encoders with the reference's channel counts (n_downsample = 2):

  fnet   BasicEncoder(output_dim=256, norm_fn='instance') on the pair: 2B images.  stem 7x7 3 -> 64 at 544x960; layer1 64 -> 64;
         layer2 64 -> 96 at stride 2 (272x480); layer3 96 -> 128 at stride 2 (136x240); conv2 1x1 128 -> 256
  cnet   MultiBasicEncoder(norm_fn='batch') in eval mode on the left image: B images; the same trunk, layer4 and layer5 128 -> 128 at
         stride 2 (68x120, 34x60), two heads of (ResidualBlock, 3x3 128 -> 128) at 136x240 and at 68x120, two 3x3 at 34x60

  A   FusedEncoder(encoder)                  torch's convolutions, the glue on the device
  B   FusedEncoder(encoder, convs=True)      the same glue, the convolutions on conv_kernels.hip

The timed units: fnet and cnet whole, and single convolutions through the wrapper's own `_conv` on fnet's 2B images: the 3x3 at
stride 1 at each resolution (64 -> 64 full, 96 -> 96 half, 128 -> 128 quarter), the 3x3 at stride 2 (64 -> 96 from full, 96 -> 128
from half), the 1x1 at stride 2 (64 -> 96 from full, 96 -> 128 from half), and the heads (3x3 128 -> 128 and the 1x1 128 -> 256 at a
quarter).  float32 and bfloat16 storage, B = 1 and 4.  A and B are alternated round by round, so that a change of the machine's
state falls on both; median, minimum and maximum over the rounds are reported, and for a single convolution the TFLOP/s its
median makes (2 multiply-adds counted as the convolution defines them; "layer1_TFLOPs" is the 64 -> 64 unit's).  The times are device
events around the whole Python call and so include the host's launch cost on both sides.  "B_faster" / "A_faster" say whether the
medians differ by more than the larger of the two ranges.  Prints one JSON line and writes it to profiles/encoder_convs.json with
--write."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vppstereo_amd.engine import Engine  # noqa: E402
from tools._timing import alternate  # noqa: E402
from vppstereo_amd.extractor import FusedEncoder  # noqa: E402

H, W = 544, 960
# name: (cin, cout, ksize, stride, the input's size as a fraction of the frame)
UNITS = {"3x3_s1_full_64": (64, 64, 3, 1, 1), "3x3_s1_half_96": (96, 96, 3, 1, 2), "3x3_s1_quarter_128": (128, 128, 3, 1, 4),
         "3x3_s2_full_64_96": (64, 96, 3, 2, 1), "3x3_s2_half_96_128": (96, 128, 3, 2, 2),
         "1x1_s2_full_64_96": (64, 96, 1, 2, 1), "1x1_s2_half_96_128": (96, 128, 1, 2, 2),
         "head_3x3_quarter_128": (128, 128, 3, 1, 4), "head_1x1_quarter_128_256": (128, 256, 1, 1, 4)}


def block(norm, cin, cout, stride):
    nn = torch.nn
    b = nn.Module()
    b.conv1, b.conv2 = nn.Conv2d(cin, cout, 3, padding=1, stride=stride), nn.Conv2d(cout, cout, 3, padding=1)
    b.norm1, b.norm2 = norm(cout), norm(cout)
    b.downsample = None if stride == 1 and cin == cout else nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride), norm(cout))
    return b


def encoder(kind):
    """fnet ('instance') or cnet ('batch') with the reference's modules and channel counts."""
    nn = torch.nn
    if kind == "instance":
        norm = lambda c: nn.InstanceNorm2d(c)                                           # noqa: E731
    else:
        def norm(c):
            m = nn.BatchNorm2d(c)
            with torch.no_grad():
                m.running_mean.normal_(0, 0.5), m.running_var.uniform_(1.0, 2.0), m.weight.uniform_(0.4, 0.8), m.bias.normal_(0, 0.3)
            return m
    layer = lambda cin, cout, stride: nn.Sequential(block(norm, cin, cout, stride), block(norm, cout, cout, 1))    # noqa: E731
    enc = nn.Module()
    enc.conv1, enc.norm1 = nn.Conv2d(3, 64, 7, stride=1, padding=3), norm(64)
    enc.layer1, enc.layer2, enc.layer3 = layer(64, 64, 1), layer(64, 96, 2), layer(96, 128, 2)
    if kind == "instance":
        enc.conv2 = nn.Conv2d(128, 256, 1)
    else:
        enc.layer4, enc.layer5 = layer(128, 128, 2), layer(128, 128, 2)
        head = lambda: nn.Sequential(block(norm, 128, 128, 1), nn.Conv2d(128, 128, 3, padding=1))      # noqa: E731
        enc.outputs08, enc.outputs16 = nn.ModuleList([head(), head()]), nn.ModuleList([head(), head()])
        enc.outputs32 = nn.ModuleList([nn.Conv2d(128, 128, 3, padding=1), nn.Conv2d(128, 128, 3, padding=1)])
    for p in enc.parameters():
        p.requires_grad_(False)
    return enc.eval()


def gflop(enc, run):
    """2 multiply-adds per weight and output pixel of every convolution of one forward, the stem included: counted by hooks while
    run() takes torch's convolutions."""
    sizes = {}
    hooks = [m.register_forward_hook(lambda m_, i, o: sizes.__setitem__(m_, o.shape[0] * o.shape[2] * o.shape[3]))
             for m in enc.modules() if isinstance(m, torch.nn.Conv2d)]
    run()
    for h in hooks:
        h.remove()
    return sum(2.0 * m.weight.numel() * px for m, px in sizes.items()) / 1e9


def row(stat, flop=None):
    med, lo, hi = stat
    r = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
    if flop is not None:
        r["TFLOPs"] = round(flop / med / 1e9, 2)
    return r


def compare(st, flop=None):
    (a, alo, ahi), (b, blo, bhi) = st["A"], st["B"]
    return {"A": row(st["A"], flop), "B": row(st["B"], flop), "A_over_B": round(a / b, 3),
            "B_faster": bool(a - b > max(ahi - alo, bhi - blo)), "A_faster": bool(b - a > max(ahi - alo, bhi - blo))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3, help="forwards of a whole encoder per round")
    ap.add_argument("--unit-iters", type=int, default=10, help="calls of a single convolution per round")
    ap.add_argument("--write", action="store_true", help="also write profiles/encoder_convs.json")
    args = ap.parse_args()
    eng = Engine()
    dev = eng.device
    torch.manual_seed(23)
    out = {"pair": [H, W], "rounds": args.rounds, "iters_per_round": args.iters, "unit_iters_per_round": args.unit_iters,
           "units": {k: dict(cin=v[0], cout=v[1], ksize=v[2], stride=v[3], input=[H // v[4], W // v[4]]) for k, v in UNITS.items()}, "cases": {}}
    g = torch.Generator(device="cpu").manual_seed(29)
    for B in args.batches:
        for name, dtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
            case = {}
            with torch.no_grad():
                for net, kind, n in (("fnet", "instance", 2 * B), ("cnet", "batch", B)):
                    enc = encoder(kind).to(device=dev, dtype=dtype)
                    fused = {"A": FusedEncoder(enc), "B": FusedEncoder(enc, convs=True)}
                    x = torch.rand((n, 3, H, W), generator=g).to(device=dev, dtype=dtype)
                    st = alternate({k: (lambda k=k: fused[k](x)) for k in fused}, args.rounds, args.iters, warm_iters=1, warm=1)
                    case[net] = dict(compare(st), images=n, GFLOP=round(gflop(enc, lambda: fused["A"](x)), 1))
                    a, b = fused["A"](x), fused["B"](x)
                    flat = lambda o: [o] if hasattr(o, "shape") else [t for grp in o for t in grp]      # noqa: E731
                    case[net]["max_abs_diff_A_vs_B"] = max(float((p.float() - q.float()).abs().max().item()) for p, q in zip(flat(a), flat(b)))
                    print(f"{net} B={B} {name}: {json.dumps(case[net])}", file=sys.stderr, flush=True)
                    del enc, fused, x, a, b
                    torch.cuda.empty_cache()
                # single convolutions, on fnet's 2B images, through the wrapper's own door
                probe = encoder("instance").to(device=dev, dtype=dtype)
                fused = {"A": FusedEncoder(probe), "B": FusedEncoder(probe, convs=True)}
                for unit, (cin, cout, ks, stride, down) in UNITS.items():
                    conv = torch.nn.Conv2d(cin, cout, ks, stride=stride, padding=ks // 2).to(device=dev, dtype=dtype)
                    x = torch.randn((2 * B, cin, H // down, W // down), generator=g).to(device=dev, dtype=dtype)
                    assert FusedEncoder._conv_plain(conv, cin)
                    st = alternate({k: (lambda k=k: fused[k]._conv(conv, x, dtype)) for k in fused}, args.rounds, args.unit_iters, warm_iters=2, warm=2)
                    y = fused["B"]._conv(conv, x, dtype)
                    flop = 2.0 * conv.weight.numel() * y.shape[2] * y.shape[3] * 2 * B
                    case[unit] = dict(compare(st, flop), GFLOP=round(flop / 1e9, 2))
                    print(f"{unit} B={B} {name}: {json.dumps(case[unit])}", file=sys.stderr, flush=True)
                    del conv, x, y
                    fused["B"].forget_weights()
                    torch.cuda.empty_cache()
                case["layer1_TFLOPs"] = case["3x3_s1_full_64"]["B"]["TFLOPs"]
                del probe, fused
            out["cases"][f"B{B}_{name}"] = case
    out["device"] = eng.ctx.device_name
    print(json.dumps(out))
    if args.write:
        with open(os.path.join(ROOT, "profiles", "encoder_convs.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
