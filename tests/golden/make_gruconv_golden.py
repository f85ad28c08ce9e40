"""Golden vectors for a ConvGRU whose convolutions run on the library's kernel, produced by running the REFERENCE's own
ConvGRU.forward (models/raft_stereo/update.py:16-32) on the CPU (the tests read the recording, not the reference):

  * "a": ConvGRU(16, 32) on 5x6 maps, B = 2, two x sources of 16 channels;
  * "b": ConvGRU(16, 16) on 3x3 maps, B = 1, one x source of 16 channels.

Each is recorded for two consecutive calls, the second on the first one's h (the context and the x sources stay).  Weights
are seeded and scaled so that the gates neither all saturate nor all sit at 1/2: tests/test_gruconv_ref_cpu.py asserts that at
least a quarter of the recorded z and r lie in (0.05, 0.95).  Per case: h0, the context [cz|cr|cq], the x sources, the three
weights and biases; per call the outputs of the three convolutions (forward hooks) and the new h.  Arrays only.

Run:  python tests/golden/make_gruconv_golden.py REFERENCE_ROOT     (writes tests/golden/gruconv_cases.npz)
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

torch.manual_seed(5701)
rng = np.random.default_rng(5702)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))       # noqa: E731
out = {}
#        name  hidden  x sources  B  H  W
CASES = (("a", 16, (16, 16), 2, 5, 6), ("b", 16, (16,), 1, 3, 3))
for name, hid, xs, B, H, W in CASES:
    gru = UP.ConvGRU(hid, sum(xs)).eval()
    with torch.no_grad():
        for p in gru.parameters():            # wider than the default initialisation, so that the convolutions move the gates
            p.mul_(2.0)
    seen = {}
    for cv in ("convz", "convr", "convq"):
        getattr(gru, cv).register_forward_hook(lambda m, i, o, cv=cv: seen.__setitem__(cv, o.detach().clone()))
        out[f"{name}_{cv}_weight"] = getattr(gru, cv).weight.detach().numpy().copy()
        out[f"{name}_{cv}_bias"] = getattr(gru, cv).bias.detach().numpy().copy()
    h = t(np.tanh(rng.standard_normal((B, hid, H, W))))
    ctx = t(rng.standard_normal((B, 3 * hid, H, W)))
    x = [t(rng.standard_normal((B, c, H, W))) for c in xs]
    out[f"{name}_h0"], out[f"{name}_ctx"] = h.numpy().copy(), ctx.numpy().copy()
    for k, xk in enumerate(x):
        out[f"{name}_x{k}"] = xk.numpy().copy()
    for call in (1, 2):
        with torch.no_grad():
            h = gru(h, *ctx.split(hid, dim=1), *x)
        for cv in ("convz", "convr", "convq"):
            out[f"{name}_call{call}_{cv}_out"] = seen[cv].numpy().copy()
        out[f"{name}_h{call}"] = h.numpy().copy()

PATH = os.path.join(HERE, "gruconv_cases.npz")
np.savez_compressed(PATH, **out)
print("wrote", len(out), "arrays,", sum(a.size for a in out.values()), "cells,", os.path.getsize(PATH), "bytes")
