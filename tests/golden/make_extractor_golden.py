"""Golden vectors for the encoders' glue, produced by running the REFERENCE's own lines on the CPU (the tests read the
recording, not the reference):

  * models/raft_stereo/extractor.py:48-60 -- ResidualBlock.forward for norm_fn 'instance' and 'batch' (eval mode): 8 -> 8
    channels at stride 1 and 8 -> 16 at stride 2 with the downsample path, on 2 frames of 6x5 cells;
  * :173-197 -- BasicEncoder('instance', downsample=2).forward on a list of two images of 8x4 pixels;
  * :274-300 -- MultiBasicEncoder('batch', downsample=2).eval().forward(x, dual_inp=True, num_layers=3) on 2 images of
    16x2 pixels (layer5 still reads two cells), output_dim [[8, 8, 8], [8, 8, 8]].

Every BatchNorm's buffers and affine parameters are drawn away from (0, 1, 1, 0) and recorded.  A forward hook on every
convolution records its input (what the glue has to hand to it) and returns its output rounded to bfloat16-representable
values, which is stored as 16 bits; the reference's own lines then run on exactly those values.  An input that is another
recorded input (a downsample convolution reads what the block's conv1 reads; the heads of one scale read the same tensor)
is not stored twice: "<unit>/<conv>/in_of" names the convolution whose input it is.  Arrays only: no weights of a
convolution, no program text.

Keys:  <unit>/x* the inputs, <unit>/<conv path>/in (float32), <unit>/<conv path>/out (uint16: bfloat16 bits),
<unit>/<norm path>/{running_mean,running_var,weight,bias} (a block's downsample.1 is its norm3), <unit>/result/<i>[/<j>] the forward's return value,
<unit>/convs the convolution paths in call order.

Run:  python tests/golden/make_extractor_golden.py REFERENCE_ROOT     (writes tests/golden/extractor_cases.npz)
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

REF = sys.argv[1]                             # root of a checkout of the reference
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
_oe = types.ModuleType("opt_einsum")          # imported by the package's update.py, not used here
_oe.contract = torch.einsum
sys.modules.setdefault("opt_einsum", _oe)
warnings.filterwarnings("ignore")

import models.raft_stereo.extractor as EX  # noqa: E402

torch.manual_seed(6601)
rng = np.random.default_rng(6602)
out = {}


def bf16_round(t):
    """float32 tensor -> the nearest bfloat16 values as float32 (ties to even)."""
    return t.to(torch.bfloat16).to(torch.float32)


def bf16_bits(t):
    return (t.contiguous().view(torch.int32) >> 16).to(torch.int16).numpy().view(np.uint16).copy()


def randomise_norms(unit, model):
    """BatchNorm buffers and affine parameters away from (0, 1, 1, 0); recorded under the norm's path."""
    done = set()
    for path, m in model.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d) and id(m) not in done:          # norm3 is also downsample.1: once
            done.add(id(m))
            C = m.num_features
            with torch.no_grad():
                m.running_mean.copy_(torch.from_numpy(rng.standard_normal(C).astype(np.float32) * 0.5))
                m.running_var.copy_(torch.from_numpy(rng.uniform(0.05, 2.0, C).astype(np.float32)))
                m.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32) * rng.choice([-1.0, 1.0], C).astype(np.float32)))
                m.bias.copy_(torch.from_numpy(rng.standard_normal(C).astype(np.float32) * 0.3))
            for k in ("running_mean", "running_var", "weight", "bias"):
                out[f"{unit}/{path}/{k}"] = getattr(m, k).detach().numpy().copy()


def record(unit, model, call):
    order, inputs = [], {}

    def hook(path):
        def fn(mod, inp, res):
            x = inp[0].detach()
            same = next((p for p in order if torch.equal(inputs[p], x)), None)
            order.append(path)
            inputs[path] = x.clone()
            if same is None:
                out[f"{unit}/{path}/in"] = x.numpy().copy()
            else:
                out[f"{unit}/{path}/in_of"] = np.array(same)
            r = bf16_round(res.detach())
            out[f"{unit}/{path}/out"] = bf16_bits(r)
            return r
        return fn

    for path, m in model.named_modules():
        if isinstance(m, torch.nn.Conv2d):
            m.register_forward_hook(hook(path))
    with torch.no_grad():
        res = call(model)
    out[f"{unit}/convs"] = np.array(order)

    def store(key, v):
        if isinstance(v, (tuple, list)):
            for i, w in enumerate(v):
                store(f"{key}/{i}", w)
        else:
            out[key] = v.detach().numpy().copy()
    store(f"{unit}/result", res)


def image(*shape):
    return torch.from_numpy((rng.standard_normal(shape) * 0.6).astype(np.float32))


for norm, tag in (("instance", "in"), ("batch", "bn")):
    for (cin, cout, stride) in ((8, 8, 1), (8, 16, 2)):
        unit = f"rb_{tag}_s{stride}"
        blk = EX.ResidualBlock(cin, cout, norm, stride=stride).eval()
        randomise_norms(unit, blk)
        # the second frame of the first channels far off zero: |mean| >> std inside a plane, and frames that differ
        x = image(2, cin, 6, 5)
        x[1, :2] += 4.0
        out[f"{unit}/x"] = x.numpy().copy()
        record(unit, blk, lambda m: m(x.clone()))

basic = EX.BasicEncoder(output_dim=16, norm_fn="instance", downsample=2).eval()
pair = [image(1, 3, 8, 4), image(1, 3, 8, 4)]
out["basic/x0"], out["basic/x1"] = pair[0].numpy().copy(), pair[1].numpy().copy()
record("basic", basic, lambda m: m([p.clone() for p in pair]))

multi = EX.MultiBasicEncoder(output_dim=[[8, 8, 8], [8, 8, 8]], norm_fn="batch", downsample=2).eval()
randomise_norms("multi", multi)
xm = image(2, 3, 16, 2)
out["multi/x"] = xm.numpy().copy()
record("multi", multi, lambda m: m(xm.clone(), dual_inp=True, num_layers=3))

PATH = os.path.join(HERE, "extractor_cases.npz")
np.savez_compressed(PATH, **out)
print("wrote", len(out), "arrays,", sum(a.size for a in out.values()), "cells,", os.path.getsize(PATH), "bytes")
