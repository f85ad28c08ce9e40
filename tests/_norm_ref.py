"""Float64 referee, its derived limits and planted wrong implementations for the encoders' glue (norm_kernels.hip): the
per-plane statistics, and the norm / ReLU / residual-sum launch.

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_norm_ref_cpu.py holds the referee to the arrays the reference's
own lines produced (tests/golden/extractor_cases.npz) and shows on those very arrays that every planted mistake leaves the
limit; tests/test_gpu_norm.py and tests/test_gpu_extractor.py hold the kernels to it.

The value.  Sums over a plane are taken in extended precision (numpy's longdouble, 64 significant bits on x86) and
everything else in float64 on the float32 (or widened bfloat16) inputs: mean = S1 / n, var = max(S2 / n - mean^2, 0),
rstd = 1 / sqrt(var + eps); v = (x - mean) rstd [w + b]; relu; relu(u + v) with a residual u, normalised likewise when it
has statistics of its own.  A non-finite cell follows IEEE arithmetic: its plane's mean or rstd is NaN and so is the plane.

limit(): how far include/vppx.h's arithmetic may lie from the value.  u = 2^-53 and U = 2^-24 bound the relative error of
one correctly rounded float64 / float32 operation; (1 + 2^-10) is the project's allowance for second-order terms
(tests/_handoff_ref.py); T = 2^-126 stands in for a relative bound where a float32 result is below the smallest normal
number.  There is no atol.  With A1 = sum |x|, S2 = sum x^2 over the n cells of a plane:

  S1', S2'   n - 1 float64 additions in any order, each within u of a partial sum that is at most A1 (S2: the squares of
             float32 numbers are exact in float64 and positive):  |S1' - S1| <= n u A1,  |S2' - S2| <= n u S2.
  mean64     one division:  dm64 = n u A1 / n + u |mean|;   mean = (float)mean64:  dmean = dm64 + U |mean| (+ T)
  var64      S2'/n (n u S2 / n and one division, u S2 / n), mean64^2 (2 |mean| dm64 and one product, u mean^2), one
             subtraction (u |var|); the clamp at 0 brings it no further from a value that is >= 0:
                 dvar = (n + 1) u S2 / n + 2 |mean| dm64 + u mean^2 + u var
  rstd       t = var64 + eps: dt = dvar + u t.  sqrt and the division round once each, and d(t^-1/2) / t^-1/2 = dt / (2 t)
             to first order, (1 - dt/t)^-1/2 - 1 in full (infinite where dt >= t: nothing is promised about such a plane):
                 drstd = rstd ((1 - dt / t)^-1/2 - 1 + 2 u + U)
  apply      d = x - mean': |d' - d| <= dmean + U |d|.   v = d rstd': dv = |d| drstd + rstd (dmean + U |d|) + U |v|.
             v w + b: dv <- |w| dv + U |v w| + U |v w + b|.   relu is 1-Lipschitz and exact.   u + v: du + dv + U |u + v|.
             Every product and sum whose exact value is below T carries T.
limit_any_f32(): the same formula evaluated in float32 throughout, in any order and association -- torch's CPU kernels,
which the recording comes from, fold a frozen BatchNorm into x * alpha + beta and take variances by other routes.  u
becomes U in the statistics, and the apply's roundings are bounded against the expanded expression's absolute terms: any
evaluation of x r w - m r w + b in at most 8 operations lies within 8 U ((|x| + |m|) r |w| + |b|) of it.

bfloat16 storage: the inputs are bfloat16 values held as float32, the float32 result is rounded once, and rounding is
monotone, so a cell lies in [rne(value - limit), rne(value + limit)]: band() of tests/_referee.py.
"""
import os
from types import SimpleNamespace

import numpy as np

from _referee import (SECOND_ORDER, TINY, U, _ns, _und, band, bf16_bits, bf16_widen, classes, compare, compare_bf16, misses,  # noqa: F401
                      to_bf16)

F32, F64, LD = np.float32, np.float64, np.longdouble
U64 = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extractor_cases.npz")
EPS = 1e-5


# ---------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------
def stats(x, eps=EPS, unit=U64, unbiased=False, eps_outside=False, per_batch=False):
    """x [B,C,H,W] -> namespace(mean, rstd, dmean, drstd), each [B,C] float64: the value and the limit of the float32 pair
    the statistics call stores.  unit = U gives the limit of a float32 evaluation (limit_any_f32).  Planted: the unbiased
    variance, eps outside the square root, one set of statistics over the whole batch."""
    x = np.asarray(x, F64)
    B, C = x.shape[:2]
    axes = (0, 2, 3) if per_batch else (2, 3)
    n = x.size // C if per_batch else x.shape[2] * x.shape[3]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xl = x.astype(LD)
        S1, S2, A1 = xl.sum(axis=axes), (xl * xl).sum(axis=axes), np.abs(xl).sum(axis=axes)
        mean_l = S1 / n
        var_l = np.where(S2 / n - mean_l * mean_l < 0, 0, S2 / n - mean_l * mean_l)   # a NaN stays
        if unbiased:
            var_l = var_l * n / max(n - 1, 1)
        mean, var, S2, A1 = mean_l.astype(F64), var_l.astype(F64), S2.astype(F64), A1.astype(F64)
        rstd = 1.0 / (np.sqrt(var) + eps) if eps_outside else 1.0 / np.sqrt(var + eps)
        dm64 = unit * A1 + unit * np.abs(mean)
        dmean = dm64 + U * np.abs(mean) + _und(mean)
        dvar = (n + 1) * unit * S2 / n + 2 * np.abs(mean) * dm64 + unit * mean * mean + unit * var
        t = var + eps
        rel = (dvar + unit * t) / t
        grow = np.where(rel < 1, 1.0 / np.sqrt(np.where(rel < 1, 1 - rel, 1.0)) - 1.0, np.inf)
        drstd = rstd * (grow + 2 * unit + U)
    if per_batch:
        mean, rstd, dmean, drstd = (np.broadcast_to(a, (B, C)).copy() for a in (mean, rstd, dmean, drstd))
    return SimpleNamespace(mean=mean, rstd=rstd, dmean=dmean * SECOND_ORDER, drstd=drstd * SECOND_ORDER, eps=eps)


def stats_value(s):
    """The [B,C,2] tensor the statistics call stores, as namespace(value, limit)."""
    return _ns(np.stack([s.mean, s.rstd], axis=-1), np.stack([s.dmean, s.drstd], axis=-1))


def frozen_stats(running_mean, running_var, eps=EPS, from_batch=None, any_f32=False):
    """A frozen BatchNorm's (mean, rstd) as FusedEncoder builds them: float64 arithmetic, rounded to float32 once; the
    kernel then reads exactly these numbers, so they carry no bound.  -> namespace like stats(), [1,C].  any_f32: the exact
    1 / sqrt(running_var + eps), which a float32 evaluation reaches within three roundings (the sum, the root, the
    division).  Planted: from_batch = the tensor whose batch statistics are taken in their place (a BatchNorm left in
    training mode)."""
    if from_batch is not None:
        s = stats(from_batch, eps, per_batch=True)
        return SimpleNamespace(mean=s.mean[:1], rstd=s.rstd[:1], dmean=s.dmean[:1], drstd=s.drstd[:1], eps=eps)
    m = np.asarray(running_mean, F64).astype(F32).astype(F64)[None]
    r = (1.0 / np.sqrt(np.asarray(running_var, F64) + eps))[None]
    if any_f32:
        return SimpleNamespace(mean=m, rstd=r, dmean=np.zeros_like(m), drstd=3 * U * r * SECOND_ORDER, eps=eps)
    r = r.astype(F32).astype(F64)
    return SimpleNamespace(mean=m, rstd=r, dmean=np.zeros_like(m), drstd=np.zeros_like(r), eps=eps)


# ---------------------------------------------------------------------------------------------------
# apply
# ---------------------------------------------------------------------------------------------------
def _bc(a, shape):
    """[B,C] or [1,C] or [C] -> broadcast over [B,C,H,W]."""
    a = np.asarray(a, F64)
    a = a[None] if a.ndim == 1 else a
    return np.broadcast_to(a[:, :, None, None], shape)


def _times(a, bound):
    """a * bound, and 0 where the bound is 0: statistics that are given carry none, whatever the cell holds."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(bound == 0, 0.0, a * bound)


def _normed(x, s, weight, bias, any_f32):
    """(x - mean) rstd [w + b] -> (value, limit)."""
    x = np.asarray(x, F64)
    m, r, dm, dr = (_bc(a, x.shape) for a in (s.mean, s.rstd, s.dmean, s.drstd))
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - m
        v = d * r
        w = _bc(weight, x.shape) if weight is not None else None
        b = _bc(bias, x.shape) if weight is not None else None
        if any_f32:
            aw = np.abs(w) if w is not None else 1.0
            val = v * w + b if w is not None else v
            lim = aw * (_times(np.abs(d), dr) + r * dm) + 8 * U * ((np.abs(x) + np.abs(m)) * r * aw + (np.abs(b) if b is not None else 0.0)) + _und(val)
            return val, lim
        lim = _times(np.abs(d), dr) + r * (dm + U * np.abs(d)) + U * np.abs(v) + _und(v)
        if w is not None:
            p = v * w
            v2 = p + b
            lim = np.abs(w) * lim + U * np.abs(p) + U * np.abs(v2) + _und(p) + _und(v2)
            v = v2
        return v, lim


def relu(v):
    with np.errstate(invalid="ignore"):
        return np.where(v < 0, 0.0, v)                  # a NaN stays


def apply(x, s, weight=None, bias=None, relu_inner=True, res=None, res_stats=None, res_weight=None, res_bias=None, res_limit=None,
          any_f32=False, relu_first=False):
    """-> namespace(value, limit) [B,C,H,W].  s / res_stats: what stats() or frozen_stats() return.  res_limit: the bound the
    residual itself arrives with.  Planted: relu_inner=False; relu_first applies the last ReLU to both operands before the
    sum instead of to the sum; res_stats=None on a downsample path skips norm3."""
    v, lim = _normed(x, s, weight, bias, any_f32)
    if relu_inner:
        v = relu(v)
    if res is not None:
        u = np.asarray(res, F64)
        lu = np.zeros_like(u) if res_limit is None else np.asarray(res_limit, F64)
        if res_stats is not None:
            assert res_limit is None
            u, lu = _normed(u, res_stats, res_weight, res_bias, any_f32)
        with np.errstate(invalid="ignore", over="ignore"):
            if relu_first:
                t = relu(u) + relu(v)
            else:
                t = u + v
            lim = lim + lu + U * np.abs(t) + _und(t)
            v = relu(t)
    return _ns(v, lim * SECOND_ORDER)


def limit(x, s, **kw):
    return apply(x, s, **kw).limit


def limit_any_f32(x, s, **kw):
    return apply(x, s, any_f32=True, **kw).limit


# ---------------------------------------------------------------------------------------------------
# the recording (tests/golden/extractor_cases.npz) through the referee
# ---------------------------------------------------------------------------------------------------
BLOCK_UNITS = ("rb_in_s1", "rb_in_s2", "rb_bn_s1", "rb_bn_s2")
UNITS = BLOCK_UNITS + ("basic", "multi")


def load_recording():
    return np.load(GOLDEN)


def conv_out(G, unit, path):
    """A convolution's recorded output: bfloat16-representable float32."""
    return bf16_widen(G[f"{unit}/{path}/out"]).reshape(G[f"{unit}/{path}/out"].shape)


def conv_in(G, unit, path):
    key = f"{unit}/{path}/in"
    return G[key] if key in G.files else G[f"{unit}/{str(G[f'{unit}/{path}/in_of'])}/in"]


def conv_paths(G, unit):
    return [str(p) for p in G[f"{unit}/convs"]]


def _norm_of(G, unit, norm_path, x, any_f32, plant):
    """(statistics, weight, bias) of the norm at `norm_path` applied to x: a recorded BatchNorm's frozen ones, else the
    plane's own."""
    key = f"{unit}/{norm_path}/running_mean"
    if key in G.files:
        g = lambda k: G[f"{unit}/{norm_path}/{k}"]                                      # noqa: E731
        if plant == "eps_outside":
            s = frozen_stats(g("running_mean"), g("running_var"), EPS, any_f32=any_f32)
            s.rstd = (1.0 / (np.sqrt(np.asarray(g("running_var"), F64)) + EPS))[None]
        else:
            s = frozen_stats(g("running_mean"), g("running_var"), EPS, from_batch=x if plant == "batch_stats" else None, any_f32=any_f32)
        return s, g("weight"), g("bias")
    kw = {"unbiased": dict(unbiased=True), "eps_outside": dict(eps_outside=True), "per_batch": dict(per_batch=True)}.get(plant, {})
    return stats(x, EPS, unit=U if any_f32 else U64, **kw), None, None


def block_stages(G, unit, prefix="", any_f32=True, plant=None, res=None, res_limit=None):
    """The two norm stages of one recorded ResidualBlock from the recorded OUTPUTS of its convolutions:
    -> {"<prefix>conv2": what conv2 has to be handed, "<prefix>out": the block's result}, each namespace(value, limit).
    `res`: the block's input where it is not conv1's recorded input (a test's own tensor).  plant: one of PLANTS."""
    p = lambda name: f"{prefix}{name}"                                                  # noqa: E731
    y1 = conv_out(G, unit, p("conv1"))
    s1, w1, b1 = _norm_of(G, unit, p("norm1"), y1, any_f32, plant)
    mid = apply(y1, s1, w1, b1, relu_inner=plant != "no_inner_relu", any_f32=any_f32)
    y2 = conv_out(G, unit, p("conv2"))
    s2, w2, b2 = _norm_of(G, unit, p("norm2"), y2, any_f32, plant)
    kw = dict(relu_inner=plant != "no_inner_relu", any_f32=any_f32, relu_first=plant == "relu_first")
    if f"{unit}/{p('downsample.0')}/out" in G.files:
        r = conv_out(G, unit, p("downsample.0"))
        if plant == "no_norm3":
            out = apply(y2, s2, w2, b2, res=r, **kw)
        else:
            s3, w3, b3 = _norm_of(G, unit, p("norm3"), r, any_f32, plant)         # downsample.1 is the block's norm3
            out = apply(y2, s2, w2, b2, res=r, res_stats=s3, res_weight=w3, res_bias=b3, **kw)
    else:
        x = conv_in(G, unit, p("conv1")) if res is None else res
        out = apply(y2, s2, w2, b2, res=x, res_limit=res_limit, **kw)
    return {p("conv2"): mid, p("out"): out}


PLANTS = ("unbiased", "eps_outside", "no_inner_relu", "relu_first", "no_norm3", "per_batch", "batch_stats")


def block_prefixes(G, unit):
    """The ResidualBlocks of a recorded unit, in call order: '' for a block unit, 'layer1.0.' ... for an encoder."""
    return [p[:-len("conv2")] for p in conv_paths(G, unit) if p.endswith(".conv2") or p == "conv2" and unit in BLOCK_UNITS]


def consumer_of(G, unit, prefix):
    """The convolution that reads the result of the block at `prefix`: the first one called after the block's own."""
    paths = conv_paths(G, unit)
    own = [i for i, p in enumerate(paths) if p.startswith(prefix) and p[len(prefix):] in ("conv1", "conv2", "downsample.0")]
    return paths[max(own) + 1] if max(own) + 1 < len(paths) else None


def unit_stages(G, unit, any_f32=True, plant=None):
    """Every norm-stage result of a recorded unit that the recording holds: {the path of the convolution that reads it, or
    'result': namespace(value, limit)}.  For an encoder that is the stem (conv1 -> norm1 -> relu, read by layer1.0.conv1),
    every block's conv2 input, and every block's result where a later convolution reads it."""
    out = {}
    if unit in BLOCK_UNITS:
        st = block_stages(G, unit, "", any_f32, plant)
        return {"conv2": st["conv2"], "result": st["out"]}
    y = conv_out(G, unit, "conv1")
    s, w, b = _norm_of(G, unit, "norm1", y, any_f32, plant)
    out["layer1.0.conv1"] = apply(y, s, w, b, relu_inner=plant != "no_inner_relu", any_f32=any_f32)
    for prefix in block_prefixes(G, unit):
        st = block_stages(G, unit, prefix, any_f32, plant)
        out[prefix + "conv2"] = st[prefix + "conv2"]
        nxt = consumer_of(G, unit, prefix)
        if nxt is not None:
            out[nxt] = st[prefix + "out"]
    return out


def recorded_stage(G, unit, key):
    return G[f"{unit}/result"] if key == "result" else conv_in(G, unit, key)
