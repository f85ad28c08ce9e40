"""Time of PSMNet's 3-D regularization with its stride-1 convolutions on the library's kernel
(vppstereo_amd.psmnet.FusedRegularization: each of the 16 stride-1 Conv3d(k=3, padding=1) one launch of Engine.conv3d with its
BatchNorm3d folded; the six stride-2 Conv3d and the six ConvTranspose3d in torch) against the same module in torch on the same
device, at the size of a 544x960 pair at maxdisp 192 (a [B,64,48,136,240] volume), on a module with the reference's structure and
channel counts (models/psmnet/psmnet.py:15-128: dres0 64 -> 32 -> 32, dres1 32 -> 32 -> 32, three hourglasses of 32 / 64
channels, three classifiers 32 -> 32 -> 1).

  A   the module's own forward in torch (for bfloat16: the module converted with .to(torch.bfloat16))
  B   FusedRegularization(module) on the same module and input

The timed units: the whole forward, and by kind single convolutions through the wrapper's own `_convbn` / `_conv` against torch's
Conv3d + BatchNorm3d + ReLU: 64 -> 32 and 32 -> 32 at quarter resolution, 64 -> 64 at an eighth and at a sixteenth (the
hourglass's conv2 and conv4), and the classifier's 32 -> 1 head (no norm, no ReLU), which computes 16 output channels to keep one.
float32 and bfloat16 storage, B = 1 and 2.  A and B are alternated round by round, so that a change of the machine's state falls
on both; median, minimum and maximum over the rounds are reported, and for a single convolution the TFLOP/s its median makes, next
to what the 2-D instance of the same kernel made in profiles/psm_features.json.  The times are device events around the whole
Python call and so include the host's launch cost on both sides.  "B_faster" / "A_faster" say whether the medians differ by more
than the larger of the two ranges.  Prints one JSON line and writes it to profiles/psm_conv3d.json with --write."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vppstereo_amd.corr import _engine  # noqa: E402
from vppstereo_amd.psmnet import FusedRegularization  # noqa: E402
from tools._timing import alternate  # noqa: E402
from tools.bench_encoder_convs import compare  # noqa: E402

H, W, MAXDISP = 544, 960, 192
# name: (cin, cout, a norm and a ReLU behind it, the volume's size as a fraction of the frame)
UNITS = {"quarter_64_32": (64, 32, True, 4), "quarter_32_32": (32, 32, True, 4), "eighth_64_64": (64, 64, True, 8),
         "sixteenth_64_64": (64, 64, True, 16), "quarter_32_1_head": (32, 1, False, 4)}
UNITS_2D = ("3x3_half_32", "3x3_quarter_64", "3x3_quarter_128")         # of profiles/psm_features.json


def convbn_3d(cin, cout, stride=1):
    nn = torch.nn
    bn = nn.BatchNorm3d(cout)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.5), bn.running_var.uniform_(1.0, 2.0), bn.weight.uniform_(0.4, 0.8), bn.bias.normal_(0, 0.3)
    return nn.Sequential(nn.Conv3d(cin, cout, kernel_size=3, padding=1, stride=stride, bias=False), bn)


def up(cin, cout):
    nn = torch.nn
    bn = nn.BatchNorm3d(cout)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.5), bn.running_var.uniform_(1.0, 2.0), bn.weight.uniform_(0.4, 0.8), bn.bias.normal_(0, 0.3)
    return nn.Sequential(nn.ConvTranspose3d(cin, cout, kernel_size=3, padding=1, output_padding=1, stride=2, bias=False), bn)


class Hourglass(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        nn = torch.nn
        self.conv1 = nn.Sequential(convbn_3d(n, 2 * n, 2), nn.ReLU(inplace=True))
        self.conv2 = convbn_3d(2 * n, 2 * n)
        self.conv3 = nn.Sequential(convbn_3d(2 * n, 2 * n, 2), nn.ReLU(inplace=True))
        self.conv4 = nn.Sequential(convbn_3d(2 * n, 2 * n), nn.ReLU(inplace=True))
        self.conv5, self.conv6 = up(2 * n, 2 * n), up(2 * n, n)

    def forward(self, x, presqu, postsqu):
        out = self.conv1(x)
        pre = self.conv2(out)
        pre = torch.relu_(pre + postsqu) if postsqu is not None else torch.relu_(pre)
        out = self.conv4(self.conv3(pre))
        post = torch.relu_(self.conv5(out) + (presqu if presqu is not None else pre))
        return self.conv6(post), pre, post


class Regularization(torch.nn.Module):
    """dres0 .. dres4 and classif1 .. classif3 with the reference's layout and channel counts, and psmnet.py:199-213 in torch."""

    def __init__(self, cin=64, c=32):
        super().__init__()
        nn = torch.nn
        relu = lambda: nn.ReLU(inplace=True)                                            # noqa: E731
        self.dres0 = nn.Sequential(convbn_3d(cin, c), relu(), convbn_3d(c, c), relu())
        self.dres1 = nn.Sequential(convbn_3d(c, c), relu(), convbn_3d(c, c))
        self.dres2, self.dres3, self.dres4 = Hourglass(c), Hourglass(c), Hourglass(c)
        for k in (1, 2, 3):
            setattr(self, f"classif{k}", nn.Sequential(convbn_3d(c, c), relu(), nn.Conv3d(c, 1, kernel_size=3, padding=1, stride=1, bias=False)))
        for p in self.parameters():
            p.requires_grad_(False)

    def forward(self, cost):
        cost0 = self.dres0(cost)
        cost0 = self.dres1(cost0) + cost0
        out1, pre1, post1 = self.dres2(cost0, None, None)
        out1 = out1 + cost0
        out2, pre2, post2 = self.dres3(out1, pre1, post1)
        out2 = out2 + cost0
        out3, pre3, post3 = self.dres4(out2, pre1, post2)
        out3 = out3 + cost0
        cost1 = self.classif1(out1)
        cost2 = self.classif2(out2) + cost1
        return self.classif3(out3) + cost2


def gflop(mod, run):
    """2 multiply-adds per weight and output cell of every Conv3d, per weight and input cell of every ConvTranspose3d, of one
    forward in torch -> (all of them, those of the stride-1 Conv3d)."""
    sizes = {}

    def hook(m, i, o):
        t = i[0] if isinstance(m, torch.nn.ConvTranspose3d) else o
        sizes[m] = t.shape[0] * t.shape[2] * t.shape[3] * t.shape[4]

    hooks = [m.register_forward_hook(hook) for m in mod.modules() if isinstance(m, (torch.nn.Conv3d, torch.nn.ConvTranspose3d))]
    run()
    for h in hooks:
        h.remove()
    each = {m: 2.0 * m.weight.numel() * n / 1e9 for m, n in sizes.items()}
    plain = sum(v for m, v in each.items() if isinstance(m, torch.nn.Conv3d) and tuple(m.stride) == (1, 1, 1))
    return sum(each.values()), plain


def conv2d_figures():
    """B's TFLOP/s of the 2-D instance's single convolutions, by case, from profiles/psm_features.json."""
    try:
        with open(os.path.join(ROOT, "profiles", "psm_features.json")) as f:
            cases = json.load(f)["cases"]
    except (OSError, ValueError, KeyError):
        return {}
    return {c: {u: v[u]["B"].get("TFLOPs") for u in UNITS_2D if u in v} for c, v in cases.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=1, help="whole forwards per round")
    ap.add_argument("--unit-iters", type=int, default=3, help="calls of a single convolution per round")
    ap.add_argument("--write", action="store_true", help="also write profiles/psm_conv3d.json")
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = _engine(dev)
    torch.manual_seed(41)
    D4, H4, W4 = MAXDISP // 4, H // 4, W // 4
    out = {"pair": [H, W], "maxdisp": MAXDISP, "volume": [64, D4, H4, W4], "rounds": args.rounds, "iters_per_round": args.iters,
           "unit_iters_per_round": args.unit_iters,
           "units": {k: dict(cin=v[0], cout=v[1], norm_relu=v[2], volume=[MAXDISP // v[3], H // v[3], W // v[3]]) for k, v in UNITS.items()},
           "conv2d_B_TFLOPs_from_psm_features": conv2d_figures(), "cases": {}}
    g = torch.Generator(device="cpu").manual_seed(43)
    for B in args.batches:
        for name, dtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
            case = {}
            with torch.no_grad():
                reg = Regularization().eval().to(device=dev, dtype=dtype)
                fused = FusedRegularization(reg)
                x = torch.randn((B, 64, D4, H4, W4), generator=g).to(device=dev, dtype=dtype)
                st = alternate({"A": lambda: reg(x), "B": lambda: fused(x)}, args.rounds, args.iters, warm_iters=1, warm=1)
                a, b = reg(x), fused(x)
                total, plain = gflop(reg, lambda: reg(x))
                case["whole"] = dict(compare(st), GFLOP=round(total, 1), GFLOP_stride1=round(plain, 1), launches=fused.launches(),
                                     max_abs_diff_A_vs_B=float((a.float() - b.float()).abs().max().item()), max_abs_A=float(a.float().abs().max().item()))
                print(f"whole B={B} {name}: {json.dumps(case['whole'])}", file=sys.stderr, flush=True)
                del a, b, x
                torch.cuda.empty_cache()
                for unit, (cin, cout, norm, down) in UNITS.items():
                    shape = (B, cin, MAXDISP // down, H // down, W // down)
                    xu = torch.randn(shape, generator=g).to(device=dev, dtype=dtype)
                    if norm:
                        pair = convbn_3d(cin, cout).eval().to(device=dev, dtype=dtype)
                        fa, fb = (lambda: torch.relu_(pair(xu))), (lambda: fused._convbn(eng, pair, xu, relu=True))
                        weights = pair[0].weight.numel()
                    else:
                        pair = torch.nn.Conv3d(cin, cout, kernel_size=3, padding=1, bias=False).eval().to(device=dev, dtype=dtype)
                        fa, fb = (lambda: pair(xu)), (lambda: fused._conv(eng, pair, xu))
                        weights = pair.weight.numel()
                    st = alternate({"A": fa, "B": fb}, args.rounds, args.unit_iters, warm_iters=2, warm=2)
                    flop = 2.0 * weights * B * shape[2] * shape[3] * shape[4]
                    case[unit] = dict(compare(st, flop), GFLOP=round(flop / 1e9, 2),
                                      max_abs_diff_A_vs_B=float((fa().float() - fb().float()).abs().max().item()))
                    print(f"{unit} B={B} {name}: {json.dumps(case[unit])}", file=sys.stderr, flush=True)
                    del pair, xu
                    fused.forget_weights()
                    torch.cuda.empty_cache()
                del reg, fused
                torch.cuda.empty_cache()
            out["cases"][f"B{B}_{name}"] = case
    out["device"] = eng.ctx.device_name
    print(json.dumps(out))
    if args.write:
        with open(os.path.join(ROOT, "profiles", "psm_conv3d.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
