"""Float64 referee, input builders and planted wrong implementations for the update block's glue (gru_kernels.hip):
the assembly of hx (copy, pool2x, interp), the reset gate written over hx, and the GRU update.

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_gru_ref_cpu.py holds the referee to the arrays the
reference's own lines produced (tests/golden/gru_cases.npz) and to torch on the CPU, and shows on the very arrays the
GPU file (tests/test_gpu_gru.py) uploads that every planted mistake leaves the limit.

What is float32 and what is float64.  The source indices and weights of interp are float32, operation by operation, as
ATen computes them for align_corners = True (tests/_readout_ref.py's lin_src has them; the CPU file pins them against
torch bit for bit).  Everything else is float64 on the float32 (or widened bfloat16) inputs.

limit(): how far a float32 evaluation of include/vppx.h's arithmetic may lie from the value.  U = 2^-24 bounds the
relative error of one correctly rounded float32 operation whose result is a normal number; the factor 1 + 2^-10 is the
project's allowance for second-order terms (tests/_handoff_ref.py); there is no atol.  Below the smallest normal
float32, T = 2^-126, the format keeps no relative precision (and expf overflows where 1 / (1 + expf(-v)) would land
there): a result whose exact value is below T may come out anywhere between 0 and T, so such a term carries T instead
of a relative bound.  With pre-activations down to -100 the gates do reach that range: sigmoid(-100) = 3.7e-44.

  pool2x   value = (sum of the 9 window cells, +0 outside the map) / 9.  Eight additions and one division, each within
           U of a partial result that is at most sum |x_k| in magnitude:  limit = 9 U sum |x_k| / 9.
  interp   value = ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d) in the float32 weights.  A tap passes through two products
           and two sums (4 roundings), and l0 + l1 = 1 within U per axis, which the fifth U covers:  limit = 5 U M, M the
           largest |tap|.
  copy     exact.
  a source that carries a bound of its own (the hidden state one GRU hands to the next) passes it on through the same
  weights: sum lim_k / 9, the lerp of the taps' bounds, the bound itself.

  v = a + c            one rounding:  dv = U |a + c|
  s = 1 / (1 + e), e = expf(-v):  ds/dv = s (1 - s) <= 1/4.  e is within 2 exp_ulps U of exp(-v'), 1 + e and the
           division round once each; the relative error of 1 + e is U + (e / (1 + e)) 2 exp_ulps U and e / (1 + e) = 1 - s:
               lim_s = s (1 - s) dv + s (2 + 2 exp_ulps (1 - s)) U          (+ T where s < T)
  t = 1 - w, w = 2 / (e + 1), e = expf(2 v'):  dt/dv = 1 - t^2 <= 1; 2 v' is exact.  w has the relative error
           2 U + (e / (e + 1)) 2 exp_ulps U with e / (e + 1) = (1 + t) / 2, and the subtraction rounds once:
               lim_t = (1 - t^2) dv + w (2 + exp_ulps (1 + t)) U + U |t|
  reset    r h:  limit = |h| lim_s + U |r h|                                 (+ T where |r h| < T)
  update   h' = (1 - z) h + z q:  1 - z, both products and the sum round once each:
               limit = (|h| + |q|) lim_z + z lim_t + U (2 |(1 - z) h| + |z q| + |h'|)    (+ T per product and result below T)
An infinite pre-activation gives its gate exactly (1 and 1, 0 and -1) in any implementation: its bound is 0.

bfloat16 storage: the inputs are bfloat16 values held as float32, the float32 result is rounded once, and rounding is
monotone, so a cell lies in [rne(value - limit), rne(value + limit)]: band(), as in tests/_handoff_bf16_ref.py.

Non-finite input follows the arithmetic (numpy's IEEE semantics) and a test compares the class of such a cell.
"""
import os
from types import SimpleNamespace

import numpy as np

import _readout_ref as R
from _referee import (SECOND_ORDER, TINY, U, _ns, _und, band, bf16_bits, bf16_widen, classes, compare, compare_bf16, misses,  # noqa: F401
                      to_bf16)

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_cases.npz")


# ---------------------------------------------------------------------------------------------------
# the assembly of hx
# ---------------------------------------------------------------------------------------------------
def pooled_size(n):
    return (n - 1) // 2 + 1


def pool2x(x, lim=None, divisor="nine", shift=0):
    """x [B,C,Hs,Ws] -> (value, limit) [B,C,(Hs-1)//2+1,(Ws-1)//2+1].  Planted: divisor="inside" divides by the number
    of window cells inside the map, shift=1 starts the window at 2y, 2x."""
    x = np.asarray(x, F64)
    B, C, Hs, Ws = x.shape
    H, W = pooled_size(Hs), pooled_size(Ws)
    lim = np.zeros_like(x) if lim is None else lim
    pad = ((0, 0), (0, 0), (1, 2), (1, 2))
    xp, ap, lp = np.pad(x, pad), np.pad(np.abs(x), pad), np.pad(lim, pad)
    cnt = np.pad(np.ones((Hs, Ws)), ((1, 2), (1, 2)))
    s = np.zeros((B, C, H, W))
    sa, sl, n = np.zeros_like(s), np.zeros_like(s), np.zeros((H, W))
    for ky in range(3):
        for kx in range(3):
            ys, xs = slice(ky + shift, ky + shift + 2 * H, 2), slice(kx + shift, kx + shift + 2 * W, 2)
            with np.errstate(invalid="ignore"):
                s = s + xp[:, :, ys, xs]
            sa, sl, n = sa + ap[:, :, ys, xs], sl + lp[:, :, ys, xs], n + cnt[ys, xs]
    d = 9.0 if divisor == "nine" else n
    with np.errstate(invalid="ignore"):
        return s / d, (U * sa * SECOND_ORDER + sl / 9.0)


def interp(x, H, W, lim=None, align_corners=True):
    """x [B,C,Hs,Ws] -> (value, limit) [B,C,H,W].  Planted: align_corners=False."""
    x = np.asarray(x, F64)
    Hs, Ws = x.shape[2:]
    lim = np.zeros_like(x) if lim is None else lim
    y0, y1, ly0, ly1 = R.lin_src(Hs, H, align_corners=align_corners)
    x0, x1, lx0, lx1 = R.lin_src(Ws, W, align_corners=align_corners)
    ly0, ly1 = ly0.astype(F64)[:, None], ly1.astype(F64)[:, None]
    lx0, lx1 = lx0.astype(F64), lx1.astype(F64)

    def lerp(a):
        r0 = a[:, :, y0][..., x0] * lx0 + a[:, :, y0][..., x1] * lx1
        r1 = a[:, :, y1][..., x0] * lx0 + a[:, :, y1][..., x1] * lx1
        return r0 * ly0 + r1 * ly1

    with np.errstate(invalid="ignore"):
        a = np.abs(x)
        M = np.maximum(np.maximum(a[:, :, y0][..., x0], a[:, :, y0][..., x1]), np.maximum(a[:, :, y1][..., x0], a[:, :, y1][..., x1]))
        return lerp(x), 5 * U * M * SECOND_ORDER + lerp(lim)


def assemble(sources, H, W):
    """sources: (array [B,C,Hs,Ws], mode) or (array, mode, bound of the array) -> namespace(value, limit) [B,sum C,H,W]."""
    vals, lims = [], []
    for src in sources:
        x, mode = np.asarray(src[0], F64), src[1]
        lim = src[2] if len(src) > 2 else None
        if mode == "copy":
            assert x.shape[2:] == (H, W)
            v, l = x, (np.zeros_like(x) if lim is None else lim)
        elif mode == "pool2x":
            v, l = pool2x(x, lim)
            assert v.shape[2:] == (H, W), (x.shape, H, W)
        else:
            v, l = interp(x, H, W, lim)
        vals.append(v), lims.append(l)
    return _ns(np.concatenate(vals, axis=1), np.concatenate(lims, axis=1))


# ---------------------------------------------------------------------------------------------------
# the gates
# ---------------------------------------------------------------------------------------------------
def _pre(a, c):
    a, c = np.asarray(a, F64), np.asarray(c, F64)
    with np.errstate(invalid="ignore"):
        v = a + c
        return v, U * np.abs(v)


def sigmoid(v, dv, exp_ulps):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = 1.0 / (1.0 + np.exp(-v))
        c = 1.0 / (1.0 + np.exp(v))                      # 1 - s without cancellation
        lim = s * c * dv + s * (2 + 2 * exp_ulps * c) * U + _und(s)
    return s, np.where(np.isfinite(v), lim, 0.0)


def tanh(v, dv, exp_ulps):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = np.tanh(v)
        w = 2.0 / (np.exp(2 * v) + 1.0)                  # 1 - t without cancellation
        lim = w * (1 + t) * dv + w * (2 + exp_ulps * (1 + t)) * U + U * np.abs(t)
    return t, np.where(np.isfinite(v), lim, 0.0)


def reset(ar, cr, h, exp_ulps=1.0, gated=True):
    """-> namespace(value = sigmoid(ar + cr) * h, limit).  Planted: gated=False leaves h."""
    h = np.asarray(h, F64)
    if not gated:
        return _ns(h, np.zeros_like(h))
    r, lr = sigmoid(*_pre(ar, cr), exp_ulps)
    with np.errstate(invalid="ignore"):
        v = r * h
        return _ns(v, (np.abs(h) * lr + U * np.abs(v) + _und(v)) * SECOND_ORDER)


def update(az, cz, aq, cq, h, exp_ulps=1.0, swap_z=False, q_gate="tanh"):
    """-> namespace(value = (1 - z) h + z q, limit).  Planted: swap_z gives z h + (1 - z) q, q_gate="sigmoid"."""
    h = np.asarray(h, F64)
    vz, dvz = _pre(az, cz)
    z, lz = sigmoid(vz, dvz, exp_ulps)
    q, lq = (tanh if q_gate == "tanh" else sigmoid)(*_pre(aq, cq), exp_ulps)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        zc = 1.0 / (1.0 + np.exp(vz))                    # 1 - z without cancellation
        if swap_z:
            z, zc = zc, z
        p1, p2 = zc * h, z * q
        v = p1 + p2
        lim = (np.abs(h) + np.abs(q)) * lz + z * lq + U * (2 * np.abs(p1) + np.abs(p2) + np.abs(v)) + _und(p1) + _und(p2) + _und(v)
    return _ns(v, lim * SECOND_ORDER)


# ---------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_gru.py
# ---------------------------------------------------------------------------------------------------
# name: (B, H, W, hx_channels or None, [(C, Hs, Ws, mode, frame padding in cells)])
ASSEMBLE_CASES = {
    # 5x7: odd sizes, hx frames of 9 * 35 cells (no 16-byte route), a padded frame stride, both parities of a pooled axis
    "odd_a":   (2, 5, 7, None, [(3, 5, 7, "copy", 11), (2, 5, 7, "copy", 0), (2, 10, 14, "pool2x", 0), (2, 3, 4, "interp", 0)]),
    "odd_b":   (2, 5, 7, None, [(2, 5, 7, "copy", 0), (3, 9, 13, "pool2x", 0), (2, 1, 1, "interp", 0)]),
    # a 1x1 destination: scale 0 on both axes, a pooled 2x2 and a pooled 1x1 map
    "one":     (2, 1, 1, None, [(2, 1, 1, "copy", 0), (1, 2, 2, "pool2x", 0), (2, 1, 1, "pool2x", 0), (2, 3, 4, "interp", 0)]),
    # 8x16: everything on 16-byte boundaries, more than one workgroup
    "aligned": (2, 8, 16, None, [(8, 8, 16, "copy", 0), (4, 16, 32, "pool2x", 0), (4, 15, 31, "pool2x", 0), (8, 4, 8, "interp", 0)]),
    # hx wider than its sources (8 channels of 35 cells: frames on 16-byte boundaries, a last group that is not whole,
    # groups that straddle two sources, a copied source that starts off a boundary); channel 7 is not written
    "wide_hx": (2, 5, 7, 8, [(3, 5, 7, "copy", 5), (2, 5, 7, "copy", 0), (1, 9, 14, "pool2x", 0), (1, 3, 4, "interp", 0)]),
}


def assemble_case(name, dtype="float32"):
    """-> namespace(sources=[(parent [B, C*Hs*Ws + padding] float32, C, Hs, Ws, mode)], B, H, W, hx_channels).  A source
    tensor is parent[:, :C*Hs*Ws] seen as [B,C,Hs,Ws]: its frames are C*Hs*Ws + padding cells apart."""
    B, H, W, hxc, srcs = ASSEMBLE_CASES[name]
    rng = np.random.default_rng([4401, B, H, W, len(srcs)])
    out = []
    for (C, Hs, Ws, mode, padding) in srcs:
        parent = (rng.standard_normal((B, C * Hs * Ws + padding)) * 3).astype(F32)
        if dtype == "bfloat16":
            parent = to_bf16(parent)
        out.append((parent, C, Hs, Ws, mode))
    total = sum(s[1] for s in out)
    return SimpleNamespace(name=name, sources=out, B=B, H=H, W=W, channels=total, hx_channels=hxc or total, dtype=dtype)


def source_view(src):
    parent, C, Hs, Ws, mode = src
    return parent[:, :C * Hs * Ws].reshape(parent.shape[0], C, Hs, Ws)


def assemble_ref(c):
    return assemble([(source_view(s), s[4]) for s in c.sources], c.H, c.W)


def assemble_stride_ignored(c):
    """Planted: frame b of a source read at b * C*Hs*Ws of its buffer, as if the frames were adjacent."""
    srcs = []
    for s in c.sources:
        parent, C, Hs, Ws, mode = s
        flat = parent.reshape(-1)[:parent.shape[0] * C * Hs * Ws]
        srcs.append((flat.reshape(parent.shape[0], C, Hs, Ws), mode))
    return assemble(srcs, c.H, c.W).value


#           name    B  C  H  W
GATE_CASES = {"c3_5x7": (2, 3, 5, 7), "c8_8x16": (2, 8, 8, 16)}
# (tensor, b, c, y, x, value) planted into the pre-activations and the state; the last two rows: h = +inf under z = 1/2,
# and both infinities under one gate
GATE_PLANTS = (("az", 0, 0, 0, 1, np.inf), ("az", 0, 1, 1, 2, -np.inf), ("az", 1, 2, 2, 0, np.nan),
               ("ar", 0, 0, 2, 3, np.inf), ("ar", 0, 2, 3, 4, -np.inf), ("ar", 1, 1, 0, 5, np.nan),
               ("aq", 0, 0, 4, 1, np.inf), ("aq", 1, 0, 4, 2, -np.inf), ("aq", 1, 1, 4, 3, np.nan),
               ("c", 0, 1, 3, 0, np.inf), ("c", 1, 2, 1, 1, -np.inf), ("c", 1, 0, 3, 3, np.nan),
               ("h", 1, 2, 4, 6, np.nan), ("h", 0, 2, 0, 6, np.inf), ("az", 1, 0, 0, 0, np.inf))


def gate_case(name, dtype="float32"):
    """-> namespace(az, ar, aq [B,C,H,W], c [B,3C,H,W] whose thirds are cz, cr, cq, h, x [B,2,H,W]).  Half of the
    pre-activations are drawn over [-100, 100], the other half near 0; a few cells are not finite."""
    B, C, H, W = GATE_CASES[name]
    rng = np.random.default_rng([4402, B, C, H, W])

    def pre(shape):
        wide = rng.uniform(-100, 100, shape)
        near = rng.standard_normal(shape) * 1.5
        return np.where(rng.random(shape) < 0.5, wide, near).astype(F32)

    a = {k: pre((B, C, H, W)) for k in ("az", "ar", "aq")}
    a["c"] = (pre((B, 3 * C, H, W)) * F32(0.5)).astype(F32)
    a["h"] = np.tanh(rng.standard_normal((B, C, H, W)) * 1.2).astype(F32)
    a["x"] = rng.standard_normal((B, 2, H, W)).astype(F32)
    for key, b, ch, y, x, val in GATE_PLANTS:
        a[key][b, ch, y, x] = val
    a["az"][0, 2, 0, 6], a["c"][0, 2, 0, 6] = 0.25, -0.25       # z = 1/2 over h = +inf
    a["ar"][0, 2, 0, 6], a["c"][0, C + 2, 0, 6] = 0.5, 0.0      # and r well above 0: 0 * inf would be NaN
    a["c"][1, 0, 0, 0] = -np.inf                               # +inf + -inf under one gate: NaN
    a["c"][0, C + 1, 2, 2], a["c"][1, 2 * C, 3, 5], a["c"][0, 2 * C + 1, 1, 4] = np.inf, -np.inf, np.nan    # cr and cq
    if dtype == "bfloat16":
        a = {k: to_bf16(v) for k, v in a.items()}
    c = a["c"]
    return SimpleNamespace(name=name, B=B, C=C, H=H, W=W, dtype=dtype, cz=c[:, :C], cr=c[:, C:2 * C], cq=c[:, 2 * C:], **a)


# ---------------------------------------------------------------------------------------------------
# the recording of BasicMultiUpdateBlock.forward (tests/golden/gru_cases.npz) through the referee
# ---------------------------------------------------------------------------------------------------
CALLS = ("it0", "it1", "slow")                   # two consecutive iterations and the slow-fast call of raft_stereo.py:134
CALL_FLAGS = {"it0": dict(iter08=True, iter16=True, iter32=True, update=True), "it1": dict(iter08=True, iter16=True, iter32=True, update=True),
              "slow": dict(iter08=False, iter16=False, iter32=True, update=False)}
ENCODER_CONVS = ("convc1", "convc2", "convf1", "convf2", "conv")


def load_recording():
    return np.load(GOLDEN)


def gru_ref(h, sources, cz, cr, cq, az, ar, aq, exp_ulps=1.0, h_limit=None):
    """One ConvGRU.forward around given convolution outputs: h [B,C,H,W], sources as assemble() takes them (without h),
    az / ar / aq the outputs of convz / convr / convq -> (hx, [r*h, x], the new h), each namespace(value, limit)."""
    h = np.asarray(h, F64)
    C, (H, W) = h.shape[1], h.shape[2:]
    hx = assemble([(h, "copy", np.zeros_like(h) if h_limit is None else h_limit)] + list(sources), H, W)
    r = reset(ar, cr, h, exp_ulps)
    rhx = _ns(np.concatenate([r.value, hx.value[:, C:]], axis=1), np.concatenate([r.limit, hx.limit[:, C:]], axis=1))
    return hx, rhx, update(az, cz, aq, cq, h, exp_ulps)


def block_ref(G, call, exp_ulps=1.0, old_net1_from=None, hx_order=None):
    """What the glue has to hand to every convolution of one recorded call, from the call's recorded inputs and the
    recorded OUTPUTS of the convolutions before it: name -> namespace(value, limit).  Keys: "gru32.hx", "gru32.rhx",
    "net2", "gru16.hx", ..., "net0" (the input of flow_head and mask), and the encoder's "convc1" ... "conv", whose inputs
    are corr, flow, and the ReLU (and cat) of recorded outputs, exactly.  The new state of one GRU reaches the next with
    its bound.  Planted: old_net1_from = a call whose OUTPUT net1 gru32 reads in place of this call's input (the new
    state where the old one belongs); hx_order permutes the two resampled sources of gru16's hx."""
    g = lambda k: G[f"{call}_{k}"]                                                      # noqa: E731
    flags = CALL_FLAGS[call]
    net = [_ns(g(f"net{i}_in").astype(F64), np.zeros(g(f"net{i}_in").shape)) for i in range(3)]
    inp = [np.split(g(f"inp{i}"), 3, axis=1) for i in range(3)]
    out = {}

    def gru(tag, i, sources):
        cz, cr, cq = inp[i]
        out[f"{tag}.hx"], out[f"{tag}.rhx"], net[i] = gru_ref(net[i].value, sources, cz, cr, cq, g(f"{tag}.convz_out"),
                                                              g(f"{tag}.convr_out"), g(f"{tag}.convq_out"), exp_ulps)
        out[f"net{i}"] = net[i]

    if flags["iter32"]:
        n1 = net[1] if old_net1_from is None else _ns(G[f"{old_net1_from}_net1_out"].astype(F64), net[1].limit)
        gru("gru32", 2, [(n1.value, "pool2x", n1.limit)])
    if flags["iter16"]:
        src = [(net[0].value, "pool2x", net[0].limit), (net[2].value, "interp", net[2].limit)]
        if hx_order is not None:
            src = [src[k] for k in hx_order]
        gru("gru16", 1, src)
    if flags["iter08"]:
        relu = lambda a: np.maximum(a, 0)                                              # noqa: E731
        exact = lambda a: _ns(a.astype(F64), np.zeros(a.shape))                        # noqa: E731
        out["convc1"], out["convf1"] = exact(g("corr")), exact(g("flow"))
        out["convc2"], out["convf2"] = exact(relu(g("convc1_out"))), exact(relu(g("convf1_out")))
        out["conv"] = exact(np.concatenate([relu(g("convc2_out")), relu(g("convf2_out"))], axis=1))
        zero = lambda a: np.zeros(a.shape)                                             # noqa: E731
        enc_out, flow = relu(g("conv_out")), g("flow")
        gru("gru08", 0, [(enc_out, "copy", zero(enc_out)), (flow, "copy", zero(flow)), (net[1].value, "interp", net[1].limit)])
    return out
