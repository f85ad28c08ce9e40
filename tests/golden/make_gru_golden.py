"""Golden vectors for the update block's glue, produced by running the REFERENCE's own lines on the CPU (the GPU tests
read the recording, not the reference):

  * models/raft_stereo/update.py:119-142 -- BasicMultiUpdateBlock.forward with hidden_dims = [8, 8, 8] and seeded
    weights, on maps of 5x6, 3x3 and 2x2 cells (what two stride-2 convolutions make of 5x6), B = 1;
  * through it ConvGRU.forward (:23-32), BasicMotionEncoder.forward (:79-87), pool2x (:89-90) and interp (:95-97).

Three calls are recorded (tests/_gru_ref.py CALLS): two consecutive iterations, the second on the first one's hidden
states, and the slow-fast call of raft_stereo.py:134 (iter32 alone, update=False).  Per call: the block's inputs
(net, the context's [cz|cr|cq] per level, corr, flow) and outputs, and, by forward hooks, the input and the output of
every convolution: the encoder's five, the nine gate convolutions, flow_head and mask.  Inputs that are the ReLU or the
concatenation of recorded outputs are not stored (convc2, convf2, conv), nor convr's, which is convz's.  Arrays only, no
weights.

Run:  python tests/golden/make_gru_golden.py REFERENCE_ROOT     (writes tests/golden/gru_cases.npz)
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
_oe = types.ModuleType("opt_einsum")          # imported by update.py, not used here
_oe.contract = torch.einsum
sys.modules.setdefault("opt_einsum", _oe)
warnings.filterwarnings("ignore")

import models.raft_stereo.update as UP  # noqa: E402

torch.manual_seed(5501)
HID = 8
SIZES = ((5, 6), (3, 3), (2, 2))
block = UP.BasicMultiUpdateBlock(types.SimpleNamespace(), hidden_dims=[HID, HID, HID]).eval()
with torch.no_grad():
    for p in block.parameters():              # wider than the default initialisation: gates that saturate on both sides
        p.mul_(3.0)

convs = {name: getattr(block.encoder, name) for name in ("convc1", "convc2", "convf1", "convf2", "conv")}
for lvl in ("gru08", "gru16", "gru32"):
    for cv in ("convz", "convr", "convq"):
        convs[f"{lvl}.{cv}"] = getattr(getattr(block, lvl), cv)
convs["flow_head"], convs["mask"] = block.flow_head, block.mask
seen = {}
for name, mod in convs.items():
    mod.register_forward_hook(lambda m, i, o, name=name: seen.__setitem__(name, (i[0].detach().clone(), o.detach().clone())))

out = {}
rng = np.random.default_rng(5502)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))       # noqa: E731


def record(call, net, inp, corr=None, flow=None, **flags):
    seen.clear()
    for i in range(3):
        out[f"{call}_net{i}_in"] = net[i].numpy().copy()
        out[f"{call}_inp{i}"] = inp[i].numpy().copy()
    if corr is not None:
        out[f"{call}_corr"], out[f"{call}_flow"] = corr.numpy().copy(), flow.numpy().copy()
    with torch.no_grad():
        res = block([n.clone() for n in net], [list(c.split(HID, dim=1)) for c in inp], corr, flow, **flags)
    net_out = res if not flags.get("update", True) else res[0]
    for i in range(3):
        out[f"{call}_net{i}_out"] = net_out[i].numpy().copy()
    if flags.get("update", True):
        out[f"{call}_mask"], out[f"{call}_delta"] = res[1].numpy().copy(), res[2].numpy().copy()
    for name, (i, o) in seen.items():
        if name.endswith("convr"):
            assert torch.equal(i, seen[name[:-1] + "z"][0])
        elif name not in ("convc1", "convc2", "convf1", "convf2", "conv"):
            out[f"{call}_{name}_in"] = i.numpy().copy()
        out[f"{call}_{name}_out"] = o.numpy().copy()
    return [n.clone() for n in net_out]


net = [t(np.tanh(rng.standard_normal((1, HID) + s))) for s in SIZES]
inp = [t(rng.standard_normal((1, 3 * HID) + s) * 2.0) for s in SIZES]
corr = t(rng.standard_normal((1, 36) + SIZES[0]) * 2.0)
flow = t(rng.standard_normal((1, 2) + SIZES[0]) * 3.0)
full = dict(iter08=True, iter16=True, iter32=True, update=True)
net1 = record("it0", net, inp, corr, flow, **full)
corr2 = t(rng.standard_normal((1, 36) + SIZES[0]) * 2.0)
net2 = record("it1", net1, inp, corr2, flow + t(out["it0_delta"]), **full)
record("slow", net2, inp, iter08=False, iter16=False, iter32=True, update=False)

PATH = os.path.join(HERE, "gru_cases.npz")
np.savez_compressed(PATH, **out)
print("wrote", len(out), "arrays,", sum(a.size for a in out.values()), "cells,", os.path.getsize(PATH), "bytes")
