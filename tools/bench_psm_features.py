"""Time of PSMNet's feature_extraction on the library's kernels (vppstereo_amd.psmnet.FusedFeatureExtraction: every convolution
behind the 3-channel stem one launch of Engine.conv2d with its BatchNorm folded, the pyramid pooling as one pool launch, four 1x1
launches and one assemble) against the same module in torch on the same device, at the size of a 544x960 pair (2B images), on a
module with the reference's structure and channel counts (models/psmnet/submodule.py:131-177: firstconv 3 -> 32 at stride 2;
layer1 3 blocks of 32; layer2 16 blocks of 64 at stride 2; layer3 3 blocks of 128; layer4 3 blocks of 128 at dilation 2; four
branches 128 -> 32; lastconv 320 -> 128 -> 32).

  A   the module's own forward in torch (for bfloat16: the module converted with .to(torch.bfloat16))
  B   FusedFeatureExtraction(module) on the same module and input

The timed units: the whole forward; by layer, each layer through the wrapper's own `_layer` (firstconv[2:], layer1 .. layer4,
the pyramid pooling `_tail` against torch's four branches, interpolations and cat, and lastconv); and by kind, single
convolutions with their BatchNorm (and ReLU) through the wrapper's own `_convbn`: the 3x3 at 32 channels and half resolution, at 64
and 128 channels and quarter resolution, the 128-channel 3x3 at dilation 2, the 3x3 at stride 2, the 1x1 at stride 2 and the
320 -> 128 3x3.  float32 and bfloat16 storage, B = 1 and 4.  A and B are alternated round by round, so that a change of the
machine's state falls on both; median, minimum and maximum over the rounds are reported, and for a single convolution the
TFLOP/s its median makes.  The times are device events around the whole Python call and so include the host's launch cost on
both sides.  "B_faster" / "A_faster" say whether the medians differ by more than the larger of the two ranges.  Prints one JSON
line and writes it to profiles/psm_features.json with --write."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vppstereo_amd.corr import _engine  # noqa: E402
from vppstereo_amd.psmnet import FusedFeatureExtraction  # noqa: E402
from tools._timing import alternate  # noqa: E402
from tools.bench_encoder_convs import compare, gflop  # noqa: E402

H, W = 544, 960
# name: (cin, cout, ksize, stride, dilation, the input's size as a fraction of the frame)
UNITS = {"3x3_half_32": (32, 32, 3, 1, 1, 2), "3x3_quarter_64": (64, 64, 3, 1, 1, 4), "3x3_quarter_128": (128, 128, 3, 1, 1, 4),
         "3x3_d2_quarter_128": (128, 128, 3, 1, 2, 4), "3x3_s2_half_32_64": (32, 64, 3, 2, 1, 2), "1x1_s2_half_32_64": (32, 64, 1, 2, 1, 2),
         "1x1_quarter_64_128": (64, 128, 1, 1, 1, 4), "3x3_quarter_320_128": (320, 128, 3, 1, 1, 4)}


def convbn(cin, cout, k, stride, dilation):
    nn = torch.nn
    bn = nn.BatchNorm2d(cout)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.5), bn.running_var.uniform_(1.0, 2.0), bn.weight.uniform_(0.4, 0.8), bn.bias.normal_(0, 0.3)
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride=stride, padding=dilation * (k // 2), dilation=dilation, bias=False), bn)


class Block(torch.nn.Module):
    def __init__(self, cin, cout, stride, dilation):
        super().__init__()
        self.conv1 = torch.nn.Sequential(convbn(cin, cout, 3, stride, dilation), torch.nn.ReLU(inplace=True))
        self.conv2 = convbn(cout, cout, 3, 1, dilation)
        self.downsample = convbn(cin, cout, 1, stride, 1) if stride != 1 or cin != cout else None

    def forward(self, x):
        y = self.conv2(self.conv1(x))
        y += x if self.downsample is None else self.downsample(x)
        return y


class Features(torch.nn.Module):
    """feature_extraction with the reference's layout and channel counts, in torch."""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        relu = lambda: nn.ReLU(inplace=True)                                            # noqa: E731
        self.firstconv = nn.Sequential(convbn(3, 32, 3, 2, 1), relu(), convbn(32, 32, 3, 1, 1), relu(), convbn(32, 32, 3, 1, 1), relu())
        layer = lambda cin, cout, n, stride, dil: nn.Sequential(*[Block(cin if j == 0 else cout, cout, stride if j == 0 else 1, dil)   # noqa: E731
                                                                  for j in range(n)])
        self.layer1, self.layer2 = layer(32, 32, 3, 1, 1), layer(32, 64, 16, 2, 1)
        self.layer3, self.layer4 = layer(64, 128, 3, 1, 1), layer(128, 128, 3, 1, 2)
        for k, win in zip((1, 2, 3, 4), (64, 32, 16, 8)):
            setattr(self, f"branch{k}", nn.Sequential(nn.AvgPool2d((win, win), stride=(win, win)), convbn(128, 32, 1, 1, 1), relu()))
        self.lastconv = nn.Sequential(convbn(320, 128, 3, 1, 1), relu(), nn.Conv2d(128, 32, 1, bias=False))
        for p in self.parameters():
            p.requires_grad_(False)

    def tail(self, raw, skip):
        up = [torch.nn.functional.interpolate(getattr(self, f"branch{k}")(skip), skip.shape[2:], mode="bilinear", align_corners=True)
              for k in (4, 3, 2, 1)]
        return torch.cat([raw, skip] + up, 1)

    def forward(self, x):
        raw = self.layer2(self.layer1(self.firstconv(x)))
        skip = self.layer4(self.layer3(raw))
        return self.lastconv(self.tail(raw, skip))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2, help="whole forwards, or runs of a layer, per round")
    ap.add_argument("--unit-iters", type=int, default=10, help="calls of a single convolution per round")
    ap.add_argument("--write", action="store_true", help="also write profiles/psm_features.json")
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = _engine(dev)
    torch.manual_seed(31)
    out = {"pair": [H, W], "rounds": args.rounds, "iters_per_round": args.iters, "unit_iters_per_round": args.unit_iters,
           "units": {k: dict(cin=v[0], cout=v[1], ksize=v[2], stride=v[3], dilation=v[4], input=[H // v[5], W // v[5]]) for k, v in UNITS.items()},
           "cases": {}}
    g = torch.Generator(device="cpu").manual_seed(37)
    rnd = lambda *s: torch.randn(s, generator=g)                                         # noqa: E731
    for B in args.batches:
        n = 2 * B
        for name, dtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
            case = {}
            with torch.no_grad():
                fe = Features().eval().to(device=dev, dtype=dtype)
                fused = FusedFeatureExtraction(fe)
                x = torch.rand((n, 3, H, W), generator=g).to(device=dev, dtype=dtype)
                st = alternate({"A": lambda: fe(x), "B": lambda: fused(x)}, args.rounds, args.iters, warm_iters=1, warm=1)
                a, b = fe(x), fused(x)
                case["whole"] = dict(compare(st), images=n, GFLOP=round(gflop(fe, lambda: fe(x)), 1), launches=fused.launches(),
                                     max_abs_diff_A_vs_B=float((a.float() - b.float()).abs().max().item()), max_abs_A=float(a.float().abs().max().item()))
                print(f"whole B={B} {name}: {json.dumps(case['whole'])}", file=sys.stderr, flush=True)
                del a, b, x
                # by layer: the wrapper's own doors against the module's
                H2, W2, H4, W4 = H // 2, W // 2, H // 4, W // 4
                t = lambda *s: rnd(*s).to(device=dev, dtype=dtype)                       # noqa: E731
                x2, x4_64, x4_128 = t(n, 32, H2, W2), t(n, 64, H4, W4), t(n, 128, H4, W4)
                buf = t(n, 320, H4, W4)
                raw, skip = buf[:, :64].contiguous(), buf[:, 64:192].contiguous()

                def first_b():
                    return fused._convbn(eng, fe.firstconv[4], fused._convbn(eng, fe.firstconv[2], x2, relu=True), relu=True)

                def last_b():
                    return fused._conv(eng, fe.lastconv[2], fused._convbn(eng, fe.lastconv[0], buf, relu=True))

                layers = {
                    "firstconv_2_4": (lambda: fe.firstconv[2:](x2), first_b),
                    "layer1": (lambda: fe.layer1(x2), lambda: fused._layer(eng, fe.layer1, x2)),
                    "layer2": (lambda: fe.layer2(x2), lambda: fused._layer(eng, fe.layer2, x2)),
                    "layer3": (lambda: fe.layer3(x4_64), lambda: fused._layer(eng, fe.layer3, x4_64)),
                    "layer4": (lambda: fe.layer4(x4_128), lambda: fused._layer(eng, fe.layer4, x4_128)),
                    "pyramid_pooling": (lambda: fe.tail(raw, skip), lambda: fused._tail(eng, buf)),
                    "lastconv": (lambda: fe.lastconv(buf), last_b),
                }
                for lname, (fa, fb) in layers.items():
                    st = alternate({"A": fa, "B": fb}, args.rounds, args.iters, warm_iters=1, warm=1)
                    case[lname] = dict(compare(st), GFLOP=round(gflop(fe, fa), 1))
                    print(f"{lname} B={B} {name}: {json.dumps(case[lname])}", file=sys.stderr, flush=True)
                del x2, x4_64, x4_128, buf, raw, skip
                torch.cuda.empty_cache()
                # by kind: single convolutions with their BatchNorm and ReLU
                for unit, (cin, cout, ks, stride, dil, down) in UNITS.items():
                    pair = convbn(cin, cout, ks, stride, dil).eval().to(device=dev, dtype=dtype)
                    xu = t(n, cin, H // down, W // down)
                    st = alternate({"A": lambda: torch.relu_(pair(xu)), "B": lambda: fused._convbn(eng, pair, xu, relu=True)}, args.rounds,
                                   args.unit_iters, warm_iters=2, warm=2)
                    y = fused._convbn(eng, pair, xu, relu=True)
                    flop = 2.0 * pair[0].weight.numel() * y.shape[2] * y.shape[3] * n
                    case[unit] = dict(compare(st, flop), GFLOP=round(flop / 1e9, 2))
                    print(f"{unit} B={B} {name}: {json.dumps(case[unit])}", file=sys.stderr, flush=True)
                    del pair, xu, y
                    fused.forget_weights()
                    torch.cuda.empty_cache()
                del fe, fused
                torch.cuda.empty_cache()
            out["cases"][f"B{B}_{name}"] = case
    out["device"] = eng.ctx.device_name
    print(json.dumps(out))
    if args.write:
        with open(os.path.join(ROOT, "profiles", "psm_features.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
