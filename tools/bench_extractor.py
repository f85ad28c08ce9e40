"""Time of the two encoders' glue (norm_kernels.hip through vppstereo_amd.extractor.FusedEncoder) against the reference's
lines written out in torch on the same device, at the size of a 544x960 pair:

  fnet   BasicEncoder(output_dim=256, norm_fn='instance', downsample=2) on the pair: 2B images.  64 channels at 544x960
         (conv1 and layer1), 96 at 272x480, 128 at 136x240
  cnet   MultiBasicEncoder(norm_fn='batch', downsample=2) in eval mode on the left image: B images, the same three scales and
         128 channels at 68x120 and 34x60, two heads at 136x240 and at 68x120

  fused   FusedEncoder.forward: per InstanceNorm one raft_norm_stats, per norm one raft_norm_apply that also applies the
          ReLU and, behind a block's second convolution, adds the residual (normalised on the downsample path) and applies
          the last ReLU, in place over the convolution's output
  torch   extractor.py:48-60, :181-183, :276-278 as the reference has them: the norm module, the in-place ReLU, x + y, ReLU

On BOTH sides every convolution is a stand-in that returns a preallocated tensor, so that only the glue is timed; what the
glue hands them is computed and dropped.  float32 and bfloat16, B = 1 and 4.  The two variants are alternated round by round,
so that a change of the machine's state falls on both; median, minimum and maximum over the rounds are reported, with the
bytes the fused launches have to move (the statistics read x once; the apply reads x, reads the residual where there is one
and writes once) and the rate that implies.  The times are device events around the whole Python call and so include the
host's launch cost on both sides.  "faster_beyond_ranges" says whether torch's fastest round is slower than the fused
slowest.  Prints one JSON line and writes it to profiles/extractor.json with --write."""
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


def row(stat, frames, nbytes=None):
    med, lo, hi = stat
    r = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), per_frame_ms=round(med / frames, 4))
    if nbytes is not None:
        r.update(MB_moved=round(nbytes / 1e6, 1), GBps=round(nbytes / med / 1e6, 1))
    return r


class Stand(torch.nn.Module):
    """A convolution's stand-in: returns what the convolution would, made once.  The fused glue works in place over it, as it
    does over a real convolution's output, so its values change from call to call, which the times do not depend on.  While
    `fresh` is set (the comparison of the two variants' results) it returns a copy instead and keeps what it was handed."""
    fresh = False

    def __init__(self, out):
        super().__init__()
        self.out, self.seen = out, None

    def forward(self, x):
        if Stand.fresh:
            self.seen = x
            return self.out.clone()
        return self.out


class Block(torch.nn.Module):
    def __init__(self, make, norm, n, cin, cout, h, w, stride):
        super().__init__()
        h, w = (h - 1) // stride + 1, (w - 1) // stride + 1
        self.conv1, self.conv2 = Stand(make(n, cout, h, w)), Stand(make(n, cout, h, w))
        self.norm1, self.norm2 = norm(cout), norm(cout)
        self.downsample = None if stride == 1 and cin == cout else torch.nn.Sequential(Stand(make(n, cout, h, w)), norm(cout))
        self.cells, self.shape = n * cout * h * w, (h, w)


def layer(make, norm, n, cin, cout, h, w, stride):
    first = Block(make, norm, n, cin, cout, h, w, stride)
    return torch.nn.Sequential(first, Block(make, norm, n, cout, cout, *first.shape, 1))


def encoder(kind, make, n):
    """The stand-in of fnet ('instance') or cnet ('batch'): the reference's modules with every convolution replaced."""
    if kind == "instance":
        norm = lambda c: torch.nn.InstanceNorm2d(c)                                     # noqa: E731
    else:
        def norm(c):
            m = torch.nn.BatchNorm2d(c)
            with torch.no_grad():
                # weight / sqrt(running_var) stays below 1: applied over its own output call after call, a plane stays finite
                m.running_mean.normal_(0, 0.5), m.running_var.uniform_(1.0, 2.0), m.weight.uniform_(0.4, 0.8), m.bias.normal_(0, 0.3)
            return m
    enc = torch.nn.Module()
    enc.conv1, enc.norm1 = Stand(make(n, 64, H, W)), norm(64)
    enc.layer1 = layer(make, norm, n, 64, 64, H, W, 1)
    enc.layer2 = layer(make, norm, n, 64, 96, H, W, 2)
    enc.layer3 = layer(make, norm, n, 96, 128, *enc.layer2[0].shape, 2)
    s8 = enc.layer3[0].shape
    if kind == "instance":
        enc.conv2 = Stand(make(n, 256, *s8))
        return enc.eval()
    enc.layer4 = layer(make, norm, n, 128, 128, *s8, 2)
    s16 = enc.layer4[0].shape
    enc.layer5 = layer(make, norm, n, 128, 128, *s16, 2)
    s32 = enc.layer5[0].shape
    head = lambda s: torch.nn.Sequential(Block(make, norm, n, 128, 128, *s, 1), Stand(make(n, 128, *s)))   # noqa: E731
    enc.outputs08 = torch.nn.ModuleList([head(s8), head(s8)])
    enc.outputs16 = torch.nn.ModuleList([head(s16), head(s16)])
    enc.outputs32 = torch.nn.ModuleList([Stand(make(n, 128, *s32)), Stand(make(n, 128, *s32))])
    return enc.eval()


def torch_block(blk, x):
    """ResidualBlock.forward (extractor.py:48-60)."""
    y = torch.relu_(blk.norm1(blk.conv1(x)))
    y = torch.relu_(blk.norm2(blk.conv2(y)))
    if blk.downsample is not None:
        x = blk.downsample(x)
    return torch.relu_(x + y)


def torch_forward(enc, x):
    """BasicEncoder.forward / MultiBasicEncoder.forward (extractor.py:181-197, :276-300), num_layers = 3."""
    x = torch.relu_(enc.norm1(enc.conv1(x)))
    for lay in (enc.layer1, enc.layer2, enc.layer3):
        for blk in lay:
            x = torch_block(blk, x)
    if hasattr(enc, "conv2"):
        return enc.conv2(x)
    o8 = [f[1](torch_block(f[0], x)) for f in enc.outputs08]
    y = x
    for blk in enc.layer4:
        y = torch_block(blk, y)
    o16 = [f[1](torch_block(f[0], y)) for f in enc.outputs16]
    z = y
    for blk in enc.layer5:
        z = torch_block(blk, z)
    return o8, o16, [f(z) for f in enc.outputs32], x


def blocks_of(enc):
    for name in ("layer1", "layer2", "layer3", "layer4", "layer5"):
        yield from getattr(enc, name, ())
    for name in ("outputs08", "outputs16"):
        for f in getattr(enc, name, ()):
            yield f[0]


def fused_passes(enc, instance):
    """(cells the fused launches read or write, launches): a statistics call reads its tensor once, an apply reads x, reads
    the residual where there is one and writes once."""
    st = 1 if instance else 0
    cells, launches = enc.conv1.out.numel() * (st + 2), st + 1
    for blk in blocks_of(enc):
        ds = blk.downsample is not None
        cells += blk.cells * ((st + 2) + (st + 3) + (st if ds else 0))
        launches += (st + 1) + (st + 1) + (st if ds else 0)
    return cells, launches


def torch_passes(enc, instance):
    """Whole-tensor passes of the reference's lines, counted from the code (not measured): a norm is a statistics read
    (InstanceNorm) and a read + write, an in-place ReLU a read + write, the sum two reads and a write."""
    norm = 3 if instance else 2
    cells = enc.conv1.out.numel() * (norm + 2)
    for blk in blocks_of(enc):
        cells += blk.cells * (2 * (norm + 2) + 3 + 2 + (norm if blk.downsample is not None else 0))
    return cells


def handed(enc):
    """What every stand-in was handed in the last `fresh` pass, and forgets."""
    out = []
    for m in enc.modules():
        if isinstance(m, Stand) and m.seen is not None:
            out.append(m.seen.float())
            m.seen = None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--write", action="store_true", help="also write profiles/extractor.json")
    args = ap.parse_args()
    assert args.rounds >= 5
    eng = Engine()
    dev = eng.device
    out = {"pair": [H, W], "rounds": args.rounds, "iters_per_round": args.iters, "cases": {}}
    for B in args.batches:
        for net, kind, n in (("fnet", "instance", 2 * B), ("cnet", "batch", B)):
            for name, dtype, size in (("float32", torch.float32, 4), ("bfloat16", torch.bfloat16, 2)):
                g = torch.Generator(device=dev).manual_seed(11)
                make = lambda *s: (torch.randn(s, generator=g, device=dev) * 1.5 + 0.25).to(dtype)      # noqa: E731
                enc = encoder(kind, make, n).to(dev)
                fused = FusedEncoder(enc)
                x = make(n, 3, H, W)
                with torch.no_grad():
                    Stand.fresh = True
                    fused(x)
                    a = handed(enc)
                    torch_forward(enc, x)
                    b = handed(enc)
                    assert len(a) == len(b) >= 16
                    diff = max(float((p - q).abs().max().item()) for p, q in zip(a, b))
                    del a, b
                    Stand.fresh = False
                    st = alternate({"fused": lambda: fused(x), "torch_composition": lambda: torch_forward(enc, x)}, args.rounds, args.iters, warm_iters=2, warm=2)
                cells, launches = fused_passes(enc, kind == "instance")
                case = {"images": n, "fused": row(st["fused"], B, cells * size), "torch_composition": row(st["torch_composition"], B),
                        "fused_launches": launches, "torch_MB_counted_not_measured": round(torch_passes(enc, kind == "instance") * size / 1e6, 1),
                        "torch_over_fused": round(st["torch_composition"][0] / st["fused"][0], 2),
                        "faster_beyond_ranges": bool(st["torch_composition"][1] > st["fused"][2]),
                        "max_abs_diff_vs_torch": diff}
                out["cases"][f"{net}_B{B}_{name}"] = case
                print(f"{net} B={B} {name}: {json.dumps(case)}", file=sys.stderr, flush=True)
                del enc, fused, x
                torch.cuda.empty_cache()
    out["device"] = eng.ctx.device_name
    print(json.dumps(out))
    if args.write:
        with open(os.path.join(ROOT, "profiles", "extractor.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
