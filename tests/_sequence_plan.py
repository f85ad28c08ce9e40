"""Plans, host data, runners and referees of the two sequence tests (tests/test_gpu_sequence.py, tests/test_gpu_sequence_all.py).

TEST INFRASTRUCTURE ONLY.  A plan is a list of specs (plain dicts) and the order they are called in; a spec that occurs twice is
the SAME call: same tensors, same parameters.  For every kind of call there is
    data(s)              deterministic host arrays of the call (numpy, no GPU),
    tensors(eng, s, d)   the call's device tensors and output buffers on one engine,
    run(eng, s, t, bufs) the call; returns {name: cloned output}, cloned on the current stream,
    referee(s, d, ref)   holds the fresh-engine outputs `ref` ({name: numpy}) to the referee the feature's own test uses.
tests/test_sequence_plan_cpu.py asserts, without a GPU, what the plan claims about itself and that every referee runs on the
plan's data.

The first half is the four kinds of the first sequence test (fused, split, occ, post), moved here unchanged."""
import ctypes as C
import os

import numpy as np

import oracle
import synth

import _corr_ref as CR
import _deflate as DF
import _handoff_bf16_ref as BR
import _handoff_ref as R
import _metrics_ref as MR
import _png_streams as PS
import _scale_ref as SR
import _stage_inputs as SI
import _viz_ref as VR

F32 = np.float32
DEVICE_EXP_ULPS = 1.0           # tests/test_gpu_handoff_ref.py's figure, justified there

_BS = [1, 2, 3, 5, 8, 9, 12, 13, 16]
_DS = [8, 16, 40, 64, 96, 128, 192, 256]
# the anchor of the graph-mode block: a call that recurs with other calls in between (8-path layout: B = 2, D = 64)
_ANCHOR = dict(role="anchor", kind="fused", B=2, H=32, W=96, D=64, gocc="none", rsgm=dict(p1=10, p2min=15, gamma=40, alpha=0.5, subpixel=1, uniqueness=0.95),
               vpp=dict(), seed=11, data=1)
# the call of the plan that crosses one round of the lock-step kernel: 2 x batch_quantum + 1 frames of this shape
_QUANTUM_SHAPE = (32, 330, 192)


def _penalties(rng, mode):
    if mode == "fused":   # 3 * (24 + P2max) <= 255: byte volumes, fused layout where the shape allows it
        p2min = int(rng.integers(5, 40))
        return dict(p1=int(rng.integers(1, 25)), p2min=p2min, gamma=int(rng.integers(p2min, 62)), alpha=float(rng.choice([0.0, 0.25, 0.5, 1.0])))
    if mode == "eight":   # the three-path sums no longer fit a byte: eight line-parallel paths, byte volumes
        return dict(p1=int(rng.integers(1, 25)), p2min=int(rng.integers(17, 40)), gamma=int(rng.integers(62, 120)), alpha=float(rng.choice([0.25, 0.5, 1.0])))
    return [dict(p1=60, p2min=300, gamma=400, alpha=0.5), dict(p1=20000, p2min=40000, gamma=65000, alpha=3.0)][int(rng.integers(2))]  # u16


def _random_call(rng, small, kind=None):
    kind = kind or str(rng.choice(["fused", "fused", "fused", "split", "occ", "post"]))
    B = int(rng.choice([b for b in _BS if not small or b <= 8]))
    H = int(rng.integers(8, 33 if small else 65))
    W = int(rng.integers(16, 161 if small else 331))
    D = int(rng.choice([d for d in _DS if not small or d <= 128]))
    s = dict(kind=kind, B=B, H=H, W=W, D=D, seed=int(rng.integers(0, 1 << 16)), data=int(rng.integers(0, 1 << 16)))
    rk = _penalties(rng, str(rng.choice(["fused", "fused", "eight", "u16"])))
    rk.update(subpixel=int(rng.integers(2)), uniqueness=float(rng.choice([0.95, 0.8, 1.0])))
    s["rsgm"] = rk
    s["vpp"] = dict(wsize=int(rng.choice([1, 3, 5, 7])), direction=int(rng.integers(2)), c=float(rng.choice([0.4, 0.0, 1.0, 0.73])),
                    uniform_color=int(rng.integers(2)), c_occ=float(rng.choice([0.0, 0.2, 1.0])),
                    discard_occluded=int(rng.integers(4) == 0), interpolate=int(rng.integers(2)))
    s["gocc"] = str(rng.choice(["none", "mask", "heuristic", "params"] if kind == "fused" else ["none", "mask"]))
    s["occ"] = dict(rx=int(rng.choice([9, 17, 21])), ry=int(rng.choice([7, 13, 19])), l=float(rng.choice([2.0, 1.0])),
                    g=float(rng.choice([0.4375, 0.25])), th_conf=1.0, th_filter=float(rng.choice([0.1, 0.5])))
    return s


def _data(s):
    """Host inputs of a call (deterministic in the spec)."""
    B, H, W, D = s["B"], s["H"], s["W"], s["D"]
    rng = np.random.default_rng(s["data"])
    if s["kind"] == "post":
        Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16
        pt, pl = (Hp - H) // 2, (Wp - W) // 2
        dl = rng.uniform(1, 60, size=(B, Hp, Wp)).astype(np.float32)       # the border is cropped away
        dr = np.zeros_like(dl)
        for f in range(B):
            m = np.repeat(np.repeat(rng.uniform(1, 60, (H // 4 + 1, W // 4 + 1)), 4, 0), 4, 1)[:H, :W]
            m = (m + rng.uniform(-1, 1, m.shape) * (rng.random(m.shape) < 0.3)).astype(np.float32)
            m[rng.random(m.shape) < 0.05] = 0
            dl[f, pt:pt + H, pl:pl + W] = m
            r = np.zeros_like(m)
            ys, xs = np.nonzero(m > 0)
            xd = xs - np.rint(m[ys, xs]).astype(np.int64)
            ok = (xd >= 0) & (xd < W)
            r[ys[ok], xd[ok]] = m[ys[ok], xs[ok]]
            noise = rng.random(m.shape) < 0.05
            r[noise] = rng.uniform(0, 60, size=int(noise.sum())).astype(np.float32)
            dr[f, pt:pt + H, pl:pl + W] = r
        return dict(dl=dl, dr=dr)
    b = synth.make_batch(B, H, W, D, float(rng.choice([0.03, 0.06, 0.2])), seed=s["data"])
    d = {k: np.ascontiguousarray(b[k]) for k in ("left", "right", "hints")}
    if s["gocc"] == "mask":
        d["mask"] = ((rng.random((B, H, W)) < 0.3) & (d["hints"] > 0)).astype(np.uint8)
    return d


def _run(eng, s, t, bufs, ready=None):
    """One call of the plan on `eng` with the call's own device tensors `t` and output buffers `bufs`; returns its outputs
    (cloned on the current stream, so that a later occurrence of the same call may reuse the buffers).  ready: the inputs-ready
    event a fused call hands over (Engine.vpp_rsgm, `inputs_ready`)."""
    kind, seed = s["kind"], s["seed"]
    if kind == "post":
        o = eng.rsgm_post(t["dl"], t["dr"], s["H"], s["W"], subpixel=bool(s["rsgm"]["subpixel"]), out=bufs["out"])
        return [o.clone()]
    if kind == "occ":
        return [eng.occlusion_heuristic(t["hints"], out=bufs["occ"], **s["occ"]).clone()]
    rk = dict(s["rsgm"], dmax=s["D"])
    if kind == "split":
        lv, rv = eng.vpp(t["left"], t["right"], t["hints"], g_occ=t.get("mask"), seed=seed, **s["vpp"])
        o = eng.rsgm(t["left"], lv, rv, out=bufs["out"], **rk)
        return [o.clone(), lv, rv]
    g = {"none": None, "mask": t.get("mask"), "heuristic": "occlusion_heuristic", "params": s.get("occ")}[s["gocc"]]
    heur = s["gocc"] in ("heuristic", "params")
    o = eng.vpp_rsgm(t["left"], t["right"], t["hints"], g_occ=g, out=bufs["out"], l_vpp=bufs["lv"], r_vpp=bufs["rv"], seed=seed,
                     vpp_kw=s["vpp"], rsgm_kw=rk, occ_out=bufs["occ"] if heur else None, inputs_ready=ready)
    r = [o.clone(), bufs["lv"].clone(), bufs["rv"].clone()]
    if heur:
        r.append(bufs["occ"].clone())
    return r


def _tensors(eng, s, d):
    import torch
    t = {k: torch.from_numpy(v).to(eng.device) for k, v in d.items()}
    B, H, W = s["B"], s["H"], s["W"]
    bufs = dict(out=torch.empty((B, H, W), dtype=torch.float32, device=eng.device),
                lv=torch.empty((B, H, W, 3), dtype=torch.uint8, device=eng.device),
                rv=torch.empty((B, H, W, 3), dtype=torch.uint8, device=eng.device),
                occ=torch.empty((B, H, W), dtype=torch.uint8, device=eng.device))
    return t, bufs


def _env_engine(**env):
    from vppstereo_amd.engine import Engine
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update({k: str(v) for k, v in env.items()})
        return Engine()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _vpp_oracle_kw(v):
    """VppxVppParams fields -> the oracle's keywords."""
    return dict(wsize=v["wsize"], left2right=bool(v["direction"]), blending=v["c"], uniform_color=bool(v["uniform_color"]), c_occ=v["c_occ"],
                discard_occ=bool(v["discard_occluded"]), interpolate=bool(v["interpolate"]),
                method="maxDistance" if v.get("method") else "rnd") if v else {}


def _oracle(s, d, f):
    """The CPU oracle's outputs of frame f of call s, in the order _run returns them."""
    if s["kind"] == "post":
        Hp, Wp = d["dl"].shape[1:]
        H, W = s["H"], s["W"]
        pt, pl = (Hp - H) // 2, (Wp - W) // 2
        fd = np.ascontiguousarray(d["dl"][f, pt:pt + H, pl:pl + W])
        fdr = np.ascontiguousarray(d["dr"][f, pt:pt + H, pl:pl + W])
        fdc = fd.copy()
        fd[oracle._left_right_check(fd, fdr, 1) == 128] = 0
        fd8 = np.ascontiguousarray(fd.astype(np.uint8))
        oracle.filterSpeckles(fd8, 0, 200, 10)
        out = fd8.astype(np.float32)
        if s["rsgm"]["subpixel"]:
            keep = out != 0
            out[keep] = fdc[keep]
        out = np.ascontiguousarray(out)
        oracle._interpolate_background(out)
        return [out]
    if s["kind"] == "occ":
        return [oracle.occlusion_heuristic(d["hints"][f], **s["occ"])[1]]
    conf = None
    if s["gocc"] == "mask":
        conf = d["mask"][f]
    elif s["gocc"] == "heuristic":
        conf = oracle.occlusion_heuristic(d["hints"][f])[1]
    elif s["gocc"] == "params":
        conf = oracle.occlusion_heuristic(d["hints"][f], **s["occ"])[1]
    vk = _vpp_oracle_kw(s["vpp"])
    oracle.init_rand(s["seed"] + f)
    lo, ro = oracle.vpp(d["left"][f], d["right"][f], d["hints"][f], g_occ=conf, **vk)
    rk = dict(s["rsgm"], dmax=s["D"])
    rk["subpixel"] = bool(rk["subpixel"])
    r = [oracle.compute_rsgm(d["left"][f], lo, ro, **rk), lo, ro]
    if s["gocc"] in ("heuristic", "params"):
        r.append(conf)
    return r


# =====================================================================================================================
# every kind of call: the second plan
# =====================================================================================================================
OLD_KINDS = ("fused", "split", "occ", "post")
HOT_KINDS = ("guided", "scaled", "eval", "sampled")        # Engine.vpp_rsgm with one of its newer arguments
NEW_KINDS = HOT_KINDS + ("metrics", "viz", "sample", "handoff", "corr", "decode", "stage", "host")
ALL_KINDS = OLD_KINDS + NEW_KINDS
# kinds whose call goes through the hot path's entry: graph mode applies to them, the route lists are theirs
ROUTE_KINDS = ("fused", "split") + HOT_KINDS + ("host",)
_RK = dict(p1=10, p2min=15, gamma=40, alpha=0.5, subpixel=1, uniqueness=0.95)      # the anchor's penalties
FLOAT_MASK = np.array([0, 1, 0.5, -1], np.float32)     # the reference's float masks: the test is `> 0`


def _hold(ref, cond, *what):
    """assert cond() -- unless ref is None: a dry run of a referee (tests/test_sequence_plan_cpu.py), in which every expectation is
    computed on the plan's data and there is no output to compare it with."""
    if ref is not None:
        assert cond(), what


def hot(kind, B, H, W, D, seed, data, **kw):
    """A vpp_rsgm call.  gocc: none / mask / heuristic; guided: validhints = hints > 0 are passed; iscale, oscale; ds: disp_small is
    asked for; evaluate: gt / validgt / metrics_out / errormap; sample: None or dict(p, seed, source="src" | "gt", guided, outs);
    p_hints: the density of the hints (0: none at all, 1: every pixel)."""
    s = dict(kind=kind, B=B, H=H, W=W, D=D, seed=seed, data=data, rsgm=dict(_RK), vpp=dict(), gocc="none", guided=False, iscale=1,
             oscale=1, ds=False, evaluate=False, sample=None, p_hints=0.05)
    s.update(kw)
    if s["sample"] is not None and s["sample"]["source"] == "gt":
        assert s["evaluate"], "hints sampled from gt: the call evaluates"
    return s


def _hot_shape(s):
    return SR.scaled_shape(s["H"], s["W"], s["iscale"], s["oscale"])


def _hot_data(s):
    B, H, W, D = s["B"], s["H"], s["W"], s["D"]
    b = synth.make_batch(B, H, W, D, s["p_hints"], seed=s["data"])
    rng = np.random.default_rng([s["data"], 7])
    d = dict(left=np.ascontiguousarray(b["left"]), right=np.ascontiguousarray(b["right"]))
    h, w, _, _ = _hot_shape(s)
    if s["sample"] is None:
        d["hints"] = np.ascontiguousarray(b["hints"])
        if s["guided"]:
            d["validhints"] = (d["hints"] > 0).astype(F32)
    if s["gocc"] == "mask":
        d["mask"] = (rng.random((B, h, w)) < 0.3).astype(np.uint8)
    if s["evaluate"]:
        d["gt"] = np.ascontiguousarray(b["gt"], F32)
        d["validgt"] = rng.choice(FLOAT_MASK, size=(B, H, W), p=[0.2, 0.5, 0.2, 0.1]).astype(F32)
    if s["sample"] is not None and s["sample"]["source"] == "src":
        d["src"] = (b["gt"] + rng.normal(0, 0.5, (B, H, W))).astype(F32).clip(0.5, D - 2)
        d["validsrc"] = (rng.random((B, H, W)) < 0.6).astype(F32)
    return d


def _hot_bufs(s, empty):
    """The output buffers of a hot call: empty(shape, dtype name) -> buffer."""
    B, C = s["B"], 3
    h, w, Ho, Wo = _hot_shape(s)
    bufs = dict(out=empty((B, Ho, Wo), "float32"), lv=empty((B, h, w, C), "uint8"), rv=empty((B, h, w, C), "uint8"))
    if s["gocc"] == "heuristic":
        bufs["occ"] = empty((B, h, w), "uint8")
    if s["ds"]:
        bufs["ds"] = empty((B, h, w), "float32")
    if s["evaluate"]:
        bufs["metrics"] = empty((B, 8), "float64")
        bufs["errormap"] = empty((B, Ho, Wo), "float32")
    if s["sample"] is not None and s["sample"]["outs"]:
        bufs["hints_out"] = empty((B, s["H"], s["W"]), "float32")
        bufs["validhints_out"] = empty((B, s["H"], s["W"]), "float32")
    return bufs


def _hot_run(eng, s, t, bufs, ready=None):
    rk = dict(s["rsgm"], dmax=s["D"])
    g = {"none": None, "mask": t.get("mask"), "heuristic": "occlusion_heuristic"}[s["gocc"]]
    kw = dict(g_occ=g, out=bufs["out"], l_vpp=bufs["lv"], r_vpp=bufs["rv"], seed=s["seed"], vpp_kw=s["vpp"], rsgm_kw=rk,
              occ_out=bufs.get("occ"), iscale=s["iscale"], oscale=s["oscale"], disp_small=bufs.get("ds"), inputs_ready=ready)
    if s["evaluate"]:
        kw.update(gt=t["gt"], validgt=t["validgt"], metrics_out=bufs["metrics"], errormap=bufs["errormap"])
    if s["sample"] is not None:
        sm = s["sample"]
        smp = dict(probability=sm["p"], seed=sm["seed"], guided=sm["guided"], hints_out=bufs.get("hints_out"),
                   validhints_out=bufs.get("validhints_out"))
        if sm["source"] == "src":
            smp.update(src=t["src"], validsrc=t["validsrc"])
        eng.vpp_rsgm(t["left"], t["right"], sample=smp, **kw)
    else:
        eng.vpp_rsgm(t["left"], t["right"], t["hints"], validhints=t.get("validhints"), **kw)
    return {k: v.clone() for k, v in bufs.items()}


def cpu_sample(src, validsrc, p, seed):
    """The CPU sampler of tests/test_sample_cpu.py / test_gpu_sample_path.py: torch.manual_seed(seed); losses.sample_hints."""
    import torch
    from vppstereo_amd import losses
    torch.manual_seed(int(seed))
    h, v = losses.sample_hints(torch.from_numpy(np.array(src)), torch.from_numpy(np.array(validsrc)) > 0, p)
    return h.numpy(), v.numpy().astype(F32)


def _hot_referee(s, d, ref):
    """Frames 0 and B - 1: the composition tests/test_gpu_scale.py, test_gpu_guided.py, test_gpu_sample_path.py and
    test_gpu_metrics.py hold their calls to -- resize_u8 and torch's decimation, the CPU sampler, the oracle's occlusion
    heuristic, init_rand(seed + f), vpp, compute_rsgm at the scaled shape, the restore, oracle.guided_metrics."""
    i, o = s["iscale"], s["oscale"]
    h, w, Ho, Wo = _hot_shape(s)
    for f in sorted({0, s["B"] - 1}):
        tag = (s["kind"], f)
        l, r = d["left"][f], d["right"][f]
        if s["sample"] is not None:
            sm = s["sample"]
            src, vsrc = (d["src"], d["validsrc"]) if sm["source"] == "src" else (d["gt"], d["validgt"])
            hints, valid = cpu_sample(src[f], vsrc[f], sm["p"], (sm["seed"] + f) & 0xFFFFFFFF)
            if sm["outs"]:
                _hold(ref, lambda: np.array_equal(ref["hints_out"][f], hints) and np.array_equal(ref["validhints_out"][f], valid), tag)
            valid = valid if sm["guided"] else None
        else:
            hints, valid = d["hints"][f], (d["validhints"][f] if s["guided"] else None)
        if i != 1:
            l, r = SR.resize_u8(l, w, h), SR.resize_u8(r, w, h)
            hints = SR.scale_hints(hints, i)
            valid = SR.decimate(valid, i) if valid is not None else None
        assert hints.shape == (h, w)
        conf = d["mask"][f] if s["gocc"] == "mask" else oracle.occlusion_heuristic(hints)[1] if s["gocc"] == "heuristic" else None
        oracle.init_rand(s["seed"] + f)
        lo, ro = oracle.vpp(l, r, hints, g_occ=conf, **_vpp_oracle_kw(s["vpp"]))
        rk = dict(s["rsgm"], dmax=s["D"])
        rk["subpixel"] = bool(rk["subpixel"])
        if valid is not None:
            rk.update(hints=hints, validhints=valid)
        small = oracle.compute_rsgm(l, lo, ro, **rk)
        out = SR.restore(small, i, o)
        assert out.shape == (Ho, Wo), (tag, out.shape)
        _hold(ref, lambda: np.array_equal(ref["lv"][f], lo) and np.array_equal(ref["rv"][f], ro), tag, "patterns")
        if s["gocc"] == "heuristic":
            _hold(ref, lambda: np.array_equal(ref["occ"][f], conf), tag, "occ")
        if s["ds"]:
            _hold(ref, lambda: np.array_equal(ref["ds"][f], small), tag, "disp_small")
        _hold(ref, lambda: ref["out"][f].shape == out.shape and np.array_equal(ref["out"][f], out), tag, "out")
        if s["evaluate"]:
            gts, vs = MR.decimated_gt(d["gt"][f], d["validgt"][f], o, Ho, Wo)
            assert gts.shape == out.shape
            em = MR.numpy_errormap(out, gts, vs)
            if ref is None:
                oracle.guided_metrics(out, gts, vs)
            else:
                MR.check_record(ref["metrics"][f], out, gts, vs, tag=str(tag))
            _hold(ref, lambda: MR.same_bits(ref["errormap"][f], em), tag, "errormap")


# ---- guided_metrics alone ----------------------------------------------------------------------------------------------
def metrics(B, Ho, Wo, gt_scale, data):
    return dict(kind="metrics", B=B, Ho=Ho, Wo=Wo, gt_scale=gt_scale, data=data)


def _metrics_data(s):
    """As tests/test_gpu_metrics.py: gt at (Ho * s + a remainder below s), the float mask, disp around the decimated gt."""
    B, Ho, Wo, sc = s["B"], s["Ho"], s["Wo"], s["gt_scale"]
    rng = np.random.default_rng([s["data"], 11])
    Hg, Wg = Ho * sc + (sc - 1), Wo * sc + (sc > 1)
    gt = rng.uniform(0, 190, (B, Hg, Wg)).astype(F32)
    valid = rng.choice(FLOAT_MASK, size=(B, Hg, Wg), p=[0.3, 0.4, 0.2, 0.1]).astype(F32)
    gts, _ = MR.decimated_gt(gt, valid, sc, Ho, Wo)
    err = np.where(rng.random(gts.shape) < 0.7, rng.normal(0, 0.6, gts.shape), rng.uniform(-40, 40, gts.shape))
    return dict(disp=(gts + err).astype(F32), gt=gt, validgt=valid)


def _metrics_run(eng, s, t, bufs):
    eng.guided_metrics(t["disp"], t["gt"], t["validgt"], gt_scale=s["gt_scale"], errormap=bufs["errormap"], metrics_out=bufs["metrics"])
    return {k: v.clone() for k, v in bufs.items()}


def _metrics_referee(s, d, ref):
    gts, vs = MR.decimated_gt(d["gt"], d["validgt"], s["gt_scale"], s["Ho"], s["Wo"])
    for f in sorted({0, s["B"] - 1}):
        if ref is None:
            oracle.guided_metrics(d["disp"][f], gts[f], vs[f])
        else:
            MR.check_record(ref["metrics"][f], d["disp"][f], gts[f], vs[f], tag=f"metrics f{f}")
    em = MR.numpy_errormap(d["disp"], gts, vs)
    _hold(ref, lambda: MR.same_bits(ref["errormap"], em), "errormap")


# ---- the pictures ------------------------------------------------------------------------------------------------------
def viz(B, H, W, dilation, data):
    return dict(kind="viz", B=B, H=H, W=W, dilation=dilation, data=data)


def _viz_data(s):
    """|disp - gt| over all bins, NaN and infinities sprinkled in, the float mask; a map with infinities and a random colour
    table for colorize."""
    B, H, W = s["B"], s["H"], s["W"]
    rng = np.random.default_rng([s["data"], 13])
    n = B * H * W
    err = (rng.uniform(0, 1, n) ** 3 * 70).astype(F32)
    gt = rng.uniform(1, 60, n).astype(F32)
    disp = gt + err * rng.choice(np.array([-1, 1], F32), n)
    odd = rng.choice(n, size=max(4, n // 40), replace=False)
    disp[odd[0::4]] = np.nan
    gt[odd[1::4]] = np.nan
    disp[odd[2::4]] = np.inf
    gt[odd[3::4]] = -np.inf
    valid = rng.choice(FLOAT_MASK, n, p=[0.3, 0.4, 0.15, 0.15]).astype(F32)
    disp, gt, valid = (a.astype(F32).reshape(B, H, W) for a in (disp, gt, valid))
    with np.errstate(invalid="ignore"):
        errors = np.abs(disp - gt)
    x = rng.uniform(-50, 190, (B, H, W)).astype(F32)
    x[0].reshape(-1)[:2] = (np.inf, -np.inf)
    return dict(disp=disp, gt=gt, valid=valid, errors=errors, x=x, lut=rng.integers(0, 256, (256, 3), dtype=np.uint8))


def _viz_run(eng, s, t, bufs):
    d = s["dilation"]
    eng.error_colors(t["errors"], t["valid"], dilation=d, out=bufs["errors"])
    eng.guided_visualize(t["disp"], t["gt"], t["valid"], dilation=d, out=bufs["guided"])
    mx = eng.finite_max(t["x"])
    eng.colorize(t["x"], mx, t["lut"], dilation=d, out=bufs["colors"])
    return dict(errors=bufs["errors"].clone(), guided=bufs["guided"].clone(), max=mx, colors=bufs["colors"].clone())


def _viz_referee(s, d, ref):
    dl = s["dilation"]
    for f in sorted({0, s["B"] - 1}):
        ec = VR.error_colors(d["errors"][f], 1, d["valid"][f], True, dl)
        _hold(ref, lambda: np.array_equal(ref["errors"][f], ec), f, "error_colors")
        want = VR.guided_visualize(d["disp"][f], d["gt"][f], d["valid"][f], 1, dl)
        for n, k in enumerate(VR.KEYS):
            _hold(ref, lambda: np.array_equal(ref["guided"][n, f], want[k]), f, k)
        mx = VR.finite_max(d["x"][f])
        _hold(ref, lambda: ref["max"][f] == mx, f, "finite_max")
        col = VR.colorize(d["x"][f], mx, d["lut"], dl)
        _hold(ref, lambda: np.array_equal(ref["colors"][f], col), f, "colorize")


# ---- sample_hints alone ------------------------------------------------------------------------------------------------
def sample(B, H, W, p, seed, data):
    return dict(kind="sample", B=B, H=H, W=W, p=p, seed=seed, data=data)


def _sample_data(s):
    rng = np.random.default_rng([s["data"], 17])
    shape = (s["B"], s["H"], s["W"])
    return dict(src=rng.uniform(-3, 90, shape).astype(F32), validsrc=rng.choice(FLOAT_MASK, shape).astype(F32))


def _sample_run(eng, s, t, bufs):
    eng.sample_hints(t["src"], t["validsrc"], probability=s["p"], seed=s["seed"], out=bufs["hints"], valid_out=bufs["valid"])
    return {k: v.clone() for k, v in bufs.items()}


def _sample_referee(s, d, ref):
    for f in sorted({0, s["B"] - 1}):
        h, v = cpu_sample(d["src"][f], d["validsrc"][f], s["p"], (s["seed"] + f) & 0xFFFFFFFF)
        _hold(ref, lambda: np.array_equal(ref["hints"][f], h) and np.array_equal(ref["valid"][f], v), f)


# ---- the hand-off kernels ----------------------------------------------------------------------------------------------
def handoff(psm, raft, nchw, dtype, hints, data=0):
    """psm / raft / nchw: case names of tests/_handoff_ref.py (_handoff_bf16_ref.py for the new PSMNet shapes)."""
    return dict(kind="handoff", psm=psm, raft=raft, nchw=nchw, dtype=dtype, hints=hints, data=data)


def _psm_case(name, dtype):
    if dtype == "bfloat16":
        return BR.psm_case(name)
    return BR._build(name) if name in BR.NEW_PSM_CASES else R.psm_case(name)


def _raft_case(name, dtype):
    return BR.raft_case(name) if dtype == "bfloat16" else R.raft_case(name)


def _handoff_data(s):
    p, r = _psm_case(s["psm"], s["dtype"]), _raft_case(s["raft"], s["dtype"])
    img, mult = R.nchw_image(s["nchw"])
    rng = np.random.default_rng([s["data"], 19, r.B, r.H4, r.W2, r.W3])
    Dc = 8
    f2, f3 = rng.standard_normal((r.B, Dc, r.H4, r.W2)).astype(F32), rng.standard_normal((r.B, Dc, r.H4, r.W3)).astype(F32)
    if s["dtype"] == "bfloat16":
        f2, f3 = BR.bf16_rne_f32(f2), BR.bf16_rne_f32(f3)
    return dict(fl=p.fl, fr=p.fr, psm_hints=p.hints, psm_valid=p.valid, corr=np.ascontiguousarray(r.corr), raft_hints=r.hints,
                raft_valid=r.valid, f2=f2, f3=f3, img=img, _cases=(p, r, mult))


FEATURES = ("fl", "fr", "corr", "f2", "f3")        # the arrays of a hand-off / corr call that take the call's dtype


def _handoff_run(eng, s, t, bufs):
    import torch
    mult, h = s["_mult"], s["hints"]
    out = dict(psm=eng.psmnet_cost_volume(t["fl"], t["fr"], s["_maxdisp"], t["psm_hints"] if h else None, t["psm_valid"] if h else None))
    out["raft"] = eng.raft_corr_modulate_(t["corr"].clone(), t["raft_hints"], t["raft_valid"])
    out["whole"] = eng.raft_corr(t["f2"], t["f3"], t["raft_hints"] if h else None, t["raft_valid"] if h else None)
    out["nchw"] = eng.to_network_input(t["img"], dtype=torch.bfloat16 if s["dtype"] == "bfloat16" else torch.float32, pad_multiple=mult)
    return out


def _handoff_referee(s, d, ref):
    """ref: float32 arrays, or uint16 bits of the bfloat16 tensors."""
    p, r, mult = d["_cases"]
    bf = s["dtype"] == "bfloat16"
    pref = R.psm_volume(p.fl, p.fr, p.maxdisp, p.hints if s["hints"] else None, p.valid if s["hints"] else None, rule="library")
    rref = R.raft_modulate(r.corr, r.hints, r.valid, rule="library")
    want_nchw = R.to_nchw(d["img"], mult)[0]
    if ref is None:     # a dry run: the referee's own cells stand in for the device's
        cells = (lambda x: BR.bits(BR.bf16_rne_f32(x))) if bf else (lambda x: x)
        ref = dict(psm=cells(pref.out), raft=cells(rref.out), nchw=cells(want_nchw))
        ref["psm"] = np.where(BR.left_of_cut(pref.out.shape), ref["psm"].dtype.type(0), ref["psm"])      # (0 * factor may be -0)
    if not bf:
        if s["hints"]:
            _, beyond, changed = R.compare(ref["psm"], pref, DEVICE_EXP_ULPS)
            assert changed == 0 and beyond == 0, ("psm", s["psm"], beyond, changed)
        else:
            assert np.array_equal(ref["psm"].view(np.uint32), pref.out.view(np.uint32))
        _, beyond, changed = R.compare(ref["raft"], rref, DEVICE_EXP_ULPS)
        assert changed == 0 and beyond == 0, ("raft", s["raft"], beyond, changed)
        assert np.array_equal(ref["nchw"], want_nchw)
        if "whole" in ref:      # raft_corr: the GEMM in front, by the bound of the golden-array test
            want, lim = R.corr_whole(d["f2"], d["f3"], r.hints if s["hints"] else None, r.valid if s["hints"] else None, DEVICE_EXP_ULPS)
            with np.errstate(invalid="ignore"):
                assert (np.abs(ref["whole"].astype(np.float64) - want) <= lim).all(), ("raft_corr", s["raft"])
        return
    plain = BR.psm_plain_bits(BR.bits(p.fl), BR.bits(p.fr), p.maxdisp)
    left = BR.left_of_cut(ref["psm"].shape)
    assert (ref["psm"][left] == 0).all()
    if s["hints"]:
        keep = (pref.v == 0) & ~left
        assert np.array_equal(ref["psm"][keep], plain[keep])
        assert not (BR.outside(BR.widen(ref["psm"]), pref, DEVICE_EXP_ULPS) & ~left).any(), ("psm bf16", s["psm"])
    else:
        assert np.array_equal(ref["psm"], plain)
    keep = rref.v == 0
    assert np.array_equal(ref["raft"][keep], BR.bits(r.corr)[keep])
    assert not BR.outside(BR.widen(ref["raft"]), rref, DEVICE_EXP_ULPS).any(), ("raft bf16", s["raft"])
    assert np.array_equal(ref["nchw"], BR.bits(BR.bf16_rne_f32(want_nchw)))


# ---- the RAFT pyramid and lookup ---------------------------------------------------------------------------------------
def corr(shape, levels, radius, dtype, hints):
    return dict(kind="corr", shape=tuple(shape), levels=levels, radius=radius, dtype=dtype, hints=hints)


def _corr_data(s):
    c = CR.volume_case(s["shape"], hints=s["hints"])
    vol = BR.bf16_rne_f32(c.corr) if s["dtype"] == "bfloat16" else c.corr
    d = dict(corr=np.ascontiguousarray(vol), coords=np.ascontiguousarray(CR.coords_case(s["shape"])[0]), _cases=c)
    if s["hints"]:
        d.update(hints=c.hints, valid=c.valid)
    return d


def _corr_run(eng, s, t, bufs):
    vol = t["corr"].clone()
    pyr = eng.raft_corr_pyramid(vol, t.get("hints"), t.get("valid"), s["levels"])
    look = eng.raft_corr_lookup(pyr, t["coords"], s["radius"])
    out = {f"level{i}": lv.clone() for i, lv in enumerate(pyr)}
    out["lookup"] = look
    return out


def _corr_referee(s, d, ref):
    """Level 0 under hints to the modulation's referee (float32: R.compare; bfloat16: the band); levels 1.. to the pooling of
    what the device left at level 0, the lookup to the referee's on the device's levels: bit for bit, as tests/test_gpu_corr.py."""
    c = d["_cases"]
    bf = s["dtype"] == "bfloat16"
    if ref is None:     # a dry run: the referee's own levels and lookup stand in for the device's
        l0 = R.raft_modulate(d["corr"], c.hints, c.valid, rule="library").out if s["hints"] else d["corr"]
        pyr = CR.pyramid(BR.bits(BR.bf16_rne_f32(l0)).reshape(c.N, c.W3) if bf else l0.reshape(c.N, c.W3), s["levels"])
        ref = {f"level{i}": lv for i, lv in enumerate(pyr)}
        ref["lookup"] = CR.channels_first(CR.lookup(CR.widened(pyr), d["coords"], s["radius"]), c.B, c.H4, c.W2)
    level0 = ref["level0"].reshape(c.N, c.W3)
    if s["hints"]:
        mref = R.raft_modulate(d["corr"], c.hints, c.valid, rule="library")
        got = level0.reshape(mref.out.shape)
        if bf:
            keep = mref.v == 0
            assert np.array_equal(got[keep], BR.bits(d["corr"])[keep])
            assert not BR.outside(BR.widen(got), mref, DEVICE_EXP_ULPS).any()
        else:
            _, beyond, changed = R.compare(got, mref, DEVICE_EXP_ULPS)
            assert changed == 0 and beyond == 0, (beyond, changed)
    else:
        want0 = BR.bits(d["corr"]) if bf else d["corr"]
        assert np.array_equal(level0.view(np.uint16 if bf else np.uint32), want0.reshape(c.N, c.W3).view(np.uint16 if bf else np.uint32))
    want = CR.pyramid(level0, s["levels"])
    for i in range(1, s["levels"]):
        got = ref[f"level{i}"].reshape(c.N, c.W3 >> i)
        assert CR.same_bits(CR.widened([got])[0], CR.widened([want[i]])[0]) == 0, i
    look = CR.channels_first(CR.lookup(CR.widened(want), d["coords"], s["radius"]), c.B, c.H4, c.W2)
    assert CR.same_bits(ref["lookup"], look) == 0


# ---- the decoders ------------------------------------------------------------------------------------------------------
def decode(what, **kw):
    """what: "png" (files: names of _png_batch), "pfm" (rows, rowwords, little), "kitti" (n)."""
    return dict(kind="decode", what=what, **kw)


def _png_batch(name):
    """(files, expected samples, H, W): hand-built files of tests/_png_streams.py, three small ones or one larger one."""
    if name == "three_small":
        cs = [PS.small_good_case(k) for k in (1, 2, 3)]
    elif name == "one_stored":
        cs = [PS.stored_offsets()]
    else:
        cs = [PS.header_seams(), PS.header_seams()]
    assert len({(c.H, c.W, c.depth, c.channels) for c in cs}) == 1 and cs[0].channels == 1
    return [c.png for c in cs], [np.asarray(c.expect).reshape(c.H, c.W) for c in cs], cs[0].H, cs[0].W


def _decode_data(s):
    if s["what"] == "png":
        files, expect, H, W = _png_batch(s["files"])
        offs = np.zeros(len(files) + 1, np.int64)
        offs[1:] = np.cumsum([len(b) for b in files])
        return dict(blob=np.frombuffer(b"".join(files), np.uint8).copy(), _offs=offs, _expect=expect, _hw=(H, W))
    if s["what"] == "pfm":
        w = R.pfm_payload(s["rows"], s["rowwords"], int(s["little"]))
        return dict(raw=np.frombuffer(w.astype("<u4" if s["little"] else ">u4").tobytes(), np.uint8).copy(), _words=w)
    return dict(u16=R.kitti_samples(s["n"]).view(np.int16))


def _decode_run(eng, s, t, bufs):
    """The PNG call goes to the C entry itself: Engine.png_decode reads the status back, which synchronises."""
    from vppstereo_amd import _lib
    from vppstereo_amd.engine import _ptr
    if s["what"] == "png":
        H, W = s["_hw"]
        offs = s["_offs"]
        eng._bind_stream()
        _lib.check(eng.lib.vppx_png_decode_dev(eng.ctx.handle, len(offs) - 1, _ptr(t["blob"]), offs.ctypes.data_as(C.POINTER(C.c_int64)),
                                               H, W, 1, 1.0, _ptr(bufs["disp"]), _ptr(bufs["valid"]), None, _ptr(bufs["status"])))
        return {k: v.clone() for k, v in bufs.items()}
    if s["what"] == "pfm":
        return dict(pfm=eng.pfm_decode(t["raw"], s["rows"], s["rowwords"], 1, s["little"]))
    disp, valid = eng.kitti_disp_decode(t["u16"])
    return dict(disp=disp, valid=valid)


def _decode_referee(s, d, ref):
    if s["what"] == "png":
        _hold(ref, lambda: not ref["status"].any(), "status")
        for i, e in enumerate(d["_expect"]):
            _hold(ref, lambda: np.array_equal(ref["disp"][i], e.astype(F32)) and np.array_equal(ref["valid"][i], (e > 0).astype(np.uint8)), i)
    elif s["what"] == "pfm":
        want = R.pfm_decode_bits(d["raw"], s["rows"], s["rowwords"], 1, s["little"])
        _hold(ref, lambda: np.array_equal(ref["pfm"].view(np.uint32), want), "pfm")
    else:
        wd, wv = R.kitti_decode(d["u16"].view(np.uint16))
        _hold(ref, lambda: np.array_equal(ref["disp"], wd) and np.array_equal(ref["valid"], wv), "kitti")


# ---- the stage entries and the stage natives ---------------------------------------------------------------------------
def stage(D, H, W, B, data=3):
    """rsgm_front / rsgm_guided_rows / rsgm_mid on the cases of tests/_stage_inputs.py, and the stage natives (census, cost,
    aggregation, both WTAs, sub-pixel, median) of tests/test_gpu_rsgm.py on one frame of Hn x Wn at this D."""
    return dict(kind="stage", D=D, H=H, W=W, B=B, data=data, Hn=16, Wn=-(-max(D, 64) // 16) * 16 + 16)


def _stage_data(s):
    D, H, W, B = s["D"], s["H"], s["W"], s["B"]
    fc = SI.front_case(*SI.FRONT_SHAPES[5 + (D == 256)], 3, B, "random")     # (33, 129) or (34, 131): partly interior tiles
    gc = SI.guided_case(H, W, D, B, 5)
    Hp, Wp = SI.geom(H, W)[4:]
    mc = SI.mid_case(Hp, Wp, B)
    fr = synth.make_frame(s["Hn"], s["Wn"], D, 0.05, seed=s["data"])
    d = dict(left=np.array(fc["left"]), left_vpp=np.array(fc["left_vpp"]), right_vpp=np.array(fc["right_vpp"]),
             census_l=np.array(gc["census_l"]), census_r=np.array(gc["census_r"]), hints=np.array(gc["hints"]),
             validhints=np.array(gc["validhints"]), disp_l=np.array(mc["disp_l"]), disp_r=np.array(mc["disp_r"]),
             _gl=oracle.rgb2gray(fr["left"]), _gr=oracle.rgb2gray(fr["right"]), _cases=(fc, gc, mc))
    return d


def native_stages(mod, ctx, gl, gr, W, H, D, p=(11, 17, 0.5, 35), uniq=0.95):
    """tests/test_gpu_rsgm.py's chain of the seven natives: mod is the oracle (ctx None) or (lib, ctx handle) for the C-ABI."""
    out = dict(cl=np.zeros((H, W), np.uint32), cr=np.zeros((H, W), np.uint32), dsi=np.zeros((H, W, D), np.uint16),
               S=np.zeros((H, W, D), np.uint16), dl=np.zeros((H, W), F32), dm=np.zeros((H, W), F32), dr=np.zeros((H, W), F32))
    if ctx is None:
        mod.census5x5_SSE(gl, out["cl"], W, H)
        mod.census5x5_SSE(gr, out["cr"], W, H)
        mod.costMeasureCensus5x5_xyd_SSE(out["cl"], out["cr"], out["dsi"], W, H, D, 1)
        mod.aggregate_SSE(gl, out["dsi"], out["S"], W, H, D, p[0], p[1], p[2], p[3])
        mod.matchWTA_SSE(out["S"], out["dl"], W, H, D, uniq)
        out["dls"] = out["dl"].copy()
        mod.subPixelRefine(out["S"], out["dls"], W, H, D, 0)
        mod.median3x3_SSE(out["dls"], out["dm"], W, H)
        mod.matchWTARight_SSE(out["S"], out["dr"], W, H, D, uniq)
        return out
    from vppstereo_amd import _lib
    P = _lib.np_ptr
    ck = _lib.check
    ck(mod.vppx_census5x5(ctx, P(gl), P(out["cl"]), W, H))
    ck(mod.vppx_census5x5(ctx, P(gr), P(out["cr"]), W, H))
    ck(mod.vppx_cost_census5x5_xyd(ctx, P(out["cl"]), P(out["cr"]), P(out["dsi"]), W, H, D, 1))
    ck(mod.vppx_aggregate_img(ctx, P(gl), 1, P(out["dsi"]), P(out["S"]), W, H, D, p[0], p[1], float(p[2]), p[3]))
    ck(mod.vppx_match_wta(ctx, P(out["S"]), P(out["dl"]), W, H, D, uniq))
    out["dls"] = out["dl"].copy()
    ck(mod.vppx_subpixel_refine(ctx, P(out["S"]), P(out["dls"]), W, H, D, 0))
    ck(mod.vppx_median3x3(ctx, P(out["dls"]), P(out["dm"]), W, H))
    ck(mod.vppx_match_wta_right(ctx, P(out["S"]), P(out["dr"]), W, H, D, uniq))
    return out


def _stage_run(eng, s, t, bufs):
    import torch
    gray, cl, cr = eng.rsgm_front(t["left"], t["left_vpp"], t["right_vpp"])
    gmap, rows, count = eng.rsgm_guided_rows(t["census_l"], t["census_r"], t["hints"], t["validhints"], s["D"])
    # the rows land in the order the kernel's row counter hands them out: compared through the map, padding pixels as zeros
    flat = gmap.reshape(-1)
    owned = torch.where((flat >= 0)[:, None], rows.view(torch.int16)[flat.clamp(min=0).long()], torch.zeros((), dtype=torch.int16, device=eng.device))
    ml, mr = eng.rsgm_mid(t["disp_l"], t["disp_r"])
    out = dict(gray=gray, census_l=cl.view(torch.int32), census_r=cr.view(torch.int32), owner=(gmap >= 0), rows=owned,
               count=count.view(torch.int32), mid_l=ml, mid_r=mr)
    eng._bind_stream()
    nat = native_stages(eng.lib, eng.ctx.handle, s["_gl"], s["_gr"], s["Wn"], s["Hn"], s["D"])
    out.update({"nat_" + k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v.view(np.int16) if v.dtype == np.uint16 else v)
                for k, v in nat.items()})
    return out


def _stage_referee(s, d, ref):
    fc, gc, mc = d["_cases"]
    want = native_stages(oracle, None, d["_gl"], d["_gr"], s["Wn"], s["Hn"], s["D"])
    if ref is None:
        return
    assert np.array_equal(ref["gray"], fc["gray_left"])
    assert np.array_equal(ref["census_l"].view(np.uint32), fc["census_l"]) and np.array_equal(ref["census_r"].view(np.uint32), fc["census_r"])
    assert int(ref["count"].view(np.uint32)[0]) == gc["n"]
    owner = ref["owner"].astype(bool)
    assert np.array_equal(owner, gc["owner"])
    assert np.array_equal(ref["rows"].view(np.uint16)[owner.reshape(-1)], gc["ref_rows"])
    assert np.array_equal(ref["mid_l"], mc["ref_l"]) and np.array_equal(ref["mid_r"], mc["ref_r"])
    for k, w in want.items():
        g = ref["nat_" + k]
        assert np.array_equal(g.view(w.dtype) if g.dtype != w.dtype else g, w), k


# ---- the _host twins ---------------------------------------------------------------------------------------------------
def host(mode, B, H, W, D, seed, data, **kw):
    """mode "call": vppx_occ_vpp_rsgm_host (vppx_occ_vpp_rsgm_guided_host when guided), "scaled": vppx_occ_vpp_rsgm_scaled_host,
    "metrics": vppx_guided_metrics_host on the disparities of the same spec as a "call"."""
    s = hot("host", B, H, W, D, seed, data, **kw)
    s["mode"] = mode
    if mode == "scaled":
        s["ds"] = True
    return s


def _host_data(s):
    d = _hot_data(s)
    if s["mode"] == "metrics":
        rng = np.random.default_rng([s["data"], 23])
        d["gt"] = np.ascontiguousarray(synth.make_batch(s["B"], s["H"], s["W"], s["D"], 0.05, seed=s["data"])["gt"], F32)
        d["validgt"] = rng.choice(FLOAT_MASK, size=d["gt"].shape, p=[0.2, 0.5, 0.2, 0.1]).astype(F32)
        d["disp"] = (d["gt"] + rng.normal(0, 1.5, d["gt"].shape)).astype(F32)
    return d


def _host_run(eng, s, d):
    """The host entries on the context of `eng`: host arrays in, host arrays out, synchronous."""
    import torch
    from vppstereo_amd import _lib
    P = _lib.np_ptr
    B, H, W = s["B"], s["H"], s["W"]
    eng._bind_stream()
    if s["mode"] == "metrics":
        rec = np.zeros((B, 8), np.float64)
        em = np.zeros((B, H, W), F32)
        _lib.check(eng.lib.vppx_guided_metrics_host(eng.ctx.handle, None, B, H, W, P(d["disp"]), H, W, P(d["gt"]), P(d["validgt"]), P(rec), P(em)))
        return dict(metrics=torch.from_numpy(rec), errormap=torch.from_numpy(em))
    bufs = _hot_bufs(s, lambda shape, dt: np.zeros(shape, dt))
    heur = s["gocc"] == "heuristic"
    op = _lib.occ_params() if heur else None
    vp = _lib.vpp_params(seed=s["seed"] & 0xFFFFFFFF, **s["vpp"])
    rp = _lib.rsgm_params(**dict(s["rsgm"], dmax=s["D"]))
    head = (eng.ctx.handle, C.byref(op) if heur else None, C.byref(vp), C.byref(rp))
    pair = (B, H, W, 3, P(d["left"]), P(d["right"]), P(d["hints"]), None if heur else P(d.get("mask")))
    tail = (P(bufs.get("occ")), P(bufs["lv"]), P(bufs["rv"]), P(bufs["out"]))
    if s["mode"] == "scaled":
        sp = _lib.scale_params(iscale=s["iscale"], oscale=s["oscale"])
        _lib.check(eng.lib.vppx_occ_vpp_rsgm_scaled_host(*head, C.byref(sp), *pair, P(d.get("validhints")), *tail, P(bufs["ds"]), None))
    elif s["guided"]:
        _lib.check(eng.lib.vppx_occ_vpp_rsgm_guided_host(*head, *pair, P(d["validhints"]), *tail, None))
    else:
        _lib.check(eng.lib.vppx_occ_vpp_rsgm_host(*head, *pair, *tail, None))
    return {k: torch.from_numpy(v) for k, v in bufs.items()}


def _host_referee(s, d, ref):
    if s["mode"] != "metrics":
        return _hot_referee(s, d, ref)
    for f in sorted({0, s["B"] - 1}):
        if ref is None:
            oracle.guided_metrics(d["disp"][f], d["gt"][f], d["validgt"][f])
        else:
            MR.check_record(ref["metrics"][f], d["disp"][f], d["gt"][f], d["validgt"][f], tag=f"host metrics f{f}")
    em = MR.numpy_errormap(d["disp"], d["gt"], d["validgt"])
    _hold(ref, lambda: MR.same_bits(ref["errormap"], em), "errormap")


# ---- one interface over every kind -------------------------------------------------------------------------------------
def data(s):
    """Host arrays of a call, deterministic in the spec.  Keys that begin with an underscore stay on the host."""
    k = s["kind"]
    if k in OLD_KINDS:
        return _data(s)
    if k in HOT_KINDS:
        return _hot_data(s)
    return {"metrics": _metrics_data, "viz": _viz_data, "sample": _sample_data, "handoff": _handoff_data, "corr": _corr_data,
            "decode": _decode_data, "stage": _stage_data, "host": _host_data}[k](s)


def plan_data(specs):
    """The host data of every spec of a plan.  A spec with "shares" is the call of that role with inputs `own_in` of its own:
    every other array is the very array of the call it shares with."""
    out = []
    for s in specs:
        if "shares" in s:
            base = out[next(i for i, x in enumerate(specs) if x.get("role") == s["shares"])]
            own = data(s) if s["own_in"] else {}
            out.append(dict(base, **{k: own[k] for k in s["own_in"]}))
        else:
            out.append(data(s))
    return out


def plan_tensors(eng, specs, datas, i, cache):
    """(tensors, buffers) of spec i on `eng`; cache: {spec index: (tensors, buffers)} of this engine.  A spec with "shares" gets
    the tensors and buffers of the call it shares with -- the same pointers -- but for its inputs `own_in` and outputs `own_out`."""
    import torch
    if i not in cache:
        s = specs[i]
        if "shares" in s:
            b = next(k for k, x in enumerate(specs) if x.get("role") == s["shares"])
            t, bufs = plan_tensors(eng, specs, datas, b, cache)
            t = dict(t, **{k: torch.from_numpy(datas[i][k]).to(eng.device) for k in s["own_in"]})
            bufs = dict(bufs, **{k: torch.empty_like(bufs[k]) for k in s["own_out"]})
            cache[i] = (t, bufs)
        else:
            cache[i] = tensors(eng, s, datas[i])
    return cache[i]


def tensors(eng, s, d):
    """(device tensors of the inputs, output buffers) of a call on one engine."""
    import torch
    k = s["kind"]
    if k in OLD_KINDS:
        return _tensors(eng, s, d)
    if k == "host":
        return d, None
    dev = eng.device
    bf = s.get("dtype") == "bfloat16"
    t = {}
    for name, v in d.items():
        if name.startswith("_") or v is None:
            continue
        if bf and name in FEATURES:        # float32 values on the bf16 grid -> a bfloat16 tensor of their bits
            t[name] = torch.from_numpy(BR.bits(v).view(np.int16)).to(dev).view(torch.bfloat16)
        else:
            t[name] = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    empty = lambda shape, dt: torch.empty(shape, dtype=getattr(torch, dt), device=dev)
    if k in HOT_KINDS:
        return t, _hot_bufs(s, empty)
    if k == "metrics":
        return t, dict(metrics=empty((s["B"], 8), "float64"), errormap=empty((s["B"], s["Ho"], s["Wo"]), "float32"))
    if k == "viz":
        B, H, W = s["B"], s["H"], s["W"]
        return t, dict(errors=empty((B, H, W, 3), "uint8"), guided=empty((6, B, H, W, 3), "uint8"), colors=empty((B, H, W, 3), "uint8"))
    if k == "sample":
        return t, dict(hints=empty((s["B"], s["H"], s["W"]), "float32"), valid=empty((s["B"], s["H"], s["W"]), "float32"))
    if k == "decode" and s["what"] == "png":
        n, (H, W) = len(d["_offs"]) - 1, d["_hw"]
        return t, dict(disp=empty((n, H, W), "float32"), valid=empty((n, H, W), "uint8"), status=empty((n,), "int32"))
    return t, {}


def run(eng, s, d, t, bufs, ready=None):
    """The call on `eng`: {name: output}, device outputs cloned on the current stream.  ready: a torch.cuda.Event behind which the
    inputs of every call of the plan exist; the calls of the hot path hand it over as `inputs_ready`, so that with
    Engine.set_pipeline their front stage really starts next to the call before (without it a front stage waits for everything
    queued so far, and nothing overlaps)."""
    k = s["kind"]
    if k in OLD_KINDS:
        return {f"o{i}": x for i, x in enumerate(_run(eng, s, t, bufs, ready))}
    if k in HOT_KINDS:
        return _hot_run(eng, s, t, bufs, ready)
    if k == "host":
        return _host_run(eng, s, d)
    extra = {}
    if k == "handoff":
        extra = dict(_maxdisp=d["_cases"][0].maxdisp, _mult=d["_cases"][2])
    elif k == "decode" and s["what"] == "png":
        extra = dict(_offs=d["_offs"], _hw=d["_hw"])
    elif k == "stage":
        extra = dict(_gl=d["_gl"], _gr=d["_gr"])
    fn = {"metrics": _metrics_run, "viz": _viz_run, "sample": _sample_run, "handoff": _handoff_run, "corr": _corr_run,
          "decode": _decode_run, "stage": _stage_run}[k]
    return fn(eng, dict(s, **extra), t, bufs)


def host_array(x):
    """A tensor's cells as the referees hold them: bfloat16 as uint16 bits, everything else as it is."""
    import torch
    x = x.cpu()
    if x.dtype == torch.bfloat16:
        return x.contiguous().view(torch.int16).numpy().view(np.uint16)
    return x.numpy()


def referee(s, d, ref):
    """Holds the fresh-engine outputs of call s ({name: numpy array}) to the referee of the feature's own test.  ref None: a
    dry run -- every referee is called on the plan's data, nothing is compared."""
    k = s["kind"]
    if k in OLD_KINDS:
        for f in sorted({0, s["B"] - 1}):
            want = _oracle(s, d, f)
            _hold(ref, lambda: len(want) == len(ref), k)
            for n, w in enumerate(want):
                _hold(ref, lambda: np.array_equal(w, ref[f"o{n}"][f]), k, f, n)
        return
    if k in HOT_KINDS:
        return _hot_referee(s, d, ref)
    {"metrics": _metrics_referee, "viz": _viz_referee, "sample": _sample_referee, "handoff": _handoff_referee, "corr": _corr_referee,
     "decode": _decode_referee, "stage": _stage_referee, "host": _host_referee}[k](s, d, ref)


# ---- the plan ----------------------------------------------------------------------------------------------------------
SEEDS = (0, 1, 2)
# (name, environment, pipelined, graph mode)
CONFIGS = [
    ("default", dict(), False, False),
    ("pipelined", dict(), True, False),
    ("graph", dict(), False, True),
    ("substreams", dict(VPPX_SUBSTREAMS=2), False, False),
    ("vert0", dict(VPPX_VERT=0), False, False),
]


def _random_new(rng, k):
    """A call of one of the new kinds, drawn from the variations the issue's table asks for (all small)."""
    kind = str(rng.choice(NEW_KINDS))
    seed, dat = int(rng.integers(0, 1 << 16)), 5000 + 10 * k
    B = int(rng.choice([1, 2, 3, 5, 9]))
    H, W = int(rng.integers(24, 49)), int(rng.integers(64, 161))
    if kind == "guided":
        return hot("guided", B, H, W, int(rng.choice([8, 64, 160, 256])), seed, dat, guided=True, p_hints=float(rng.choice([0.0, 0.05, 1.0])),
                   gocc=str(rng.choice(["none", "mask", "heuristic"])))
    if kind == "scaled":
        i, o = [(2, 2), (2, 1), (3, 2), (3, 1)][int(rng.integers(4))]
        return hot("scaled", min(B, 3), 2 * (H // 2) + 1, W, 64, seed, dat, iscale=i, oscale=o, ds=True, guided=bool(rng.integers(2)),
                   gocc=str(rng.choice(["none", "heuristic"])))
    if kind == "eval":
        i, o = [(1, 1), (2, 2), (2, 1)][int(rng.integers(3))]
        return hot("eval", min(B, 3), 2 * (H // 2), 2 * (W // 2), 64, seed, dat, iscale=i, oscale=o, evaluate=True)
    if kind == "sampled":
        src = str(rng.choice(["src", "gt"]))
        return hot("sampled", min(B, 3), H, W, 64, seed, dat, evaluate=src == "gt",
                   sample=dict(p=0.05, seed=int(rng.integers(0, 1 << 32)), source=src, guided=bool(rng.integers(2)), outs=bool(rng.integers(2))))
    if kind == "metrics":
        Ho, Wo = [(37, 53), (63, 131), (64, 64), (21, 195)][int(rng.integers(4))]
        return metrics(int(rng.choice([1, 3, 4])), Ho, Wo, int(rng.choice([1, 2, 3])), dat)
    if kind == "viz":
        H, W, dl = [(5, 9, 7), (33, 130, 1), (64, 330, 0), (17, 40, 7)][int(rng.integers(4))]
        return viz(int(rng.choice([1, 3])), H, W, dl, dat)
    if kind == "sample":
        return sample(B, H, W, float(rng.choice([0.05, 1.0])), int(rng.choice([2 ** 32 - 2, 2 ** 32 - 1, 7])), dat)
    if kind == "handoff":
        return handoff(str(rng.choice(["w12", "w16_d24", "w8", "w4_d8"])), str(rng.choice(["w65", "w24_all", "w65_narrow"])),
                       str(rng.choice(["odd_pad", "c1"])), str(rng.choice(["float32", "bfloat16"])), bool(rng.integers(2)), dat)
    if kind == "corr":
        lv, rad = [(4, 4), (1, 0), (4, 0), (1, 4)][int(rng.integers(4))]
        return corr([(1, 2, 63, 17), (2, 3, 70, 37), (1, 1, 5, 30)][int(rng.integers(3))], lv, rad, str(rng.choice(["float32", "bfloat16"])),
                    bool(rng.integers(2)))
    if kind == "decode":
        what = str(rng.choice(["png", "pfm", "kitti"]))
        if what == "png":
            return decode("png", files=str(rng.choice(["three_small", "one_stored", "two_seams"])))
        if what == "pfm":
            return decode("pfm", rows=int(rng.choice([1, 9])), rowwords=int(rng.choice([255, 256, 257])), little=bool(rng.integers(2)))
        return decode("kitti", n=int(rng.choice([1, 255, 257])))
    if kind == "stage":
        return stage(int(rng.choice([64, 256])), *[(24, 48), (21, 130)][int(rng.integers(2))], int(rng.choice([1, 3])))
    mode = str(rng.choice(["call", "scaled", "metrics"]))
    if mode == "scaled":
        return host("scaled", 2, 45, 130, 64, seed, dat, iscale=2, oscale=int(rng.choice([1, 2])), guided=True, gocc="heuristic")
    return host(mode, 2, H, W, 64, seed, dat, guided=bool(rng.integers(2)), gocc=str(rng.choice(["none", "heuristic"])))


def plan(seed, quantum):
    """(specs, order, marks) of one sequence: the fixed adjacencies -- marks[name] is the list of positions of part `name` in
    the order -- and, around them, calls drawn at random from all kinds."""
    rng = np.random.default_rng(4242 + seed)
    calls, marks = [], {}

    def part(name, items):
        marks[name] = list(range(len(calls), len(calls) + len(items)))
        calls.extend(items)

    def pen(mode="fused"):
        return dict(_penalties(rng, mode), subpixel=1, uniqueness=0.95)

    tail = [_random_call(rng, True), _random_new(rng, 0)]
    # every kind occurs: the three the fixed parts do not hold come first, with a split and an occlusion call as the first plan has
    calls += [_random_call(rng, True, "split"), _random_call(rng, True, "occ"), _random_call(rng, True, "post")]
    # ... and every variation of a kind that the fixed parts below do not hold occurs once, on every seed
    part("variations", [
        viz(3, 33, 130, 7, 91), viz(1, 64, 330, 0, 93), viz(2, 5, 9, 1, 94),                    # dilation 7 / 0 / 1; larger and smaller than a tile
        sample(3, 37, 53, 0.05, 2 ** 32 - 2, 92), sample(2, 24, 40, 1.0, 2 ** 32 - 1, 95),
        decode("pfm", rows=9, rowwords=257, little=False), decode("kitti", n=257),
        host("metrics", 3, 37, 53, 64, 61, 96),
        stage(256, 21, 130, 1),
        corr((1, 1, 5, 30), 1, 0, "bfloat16", False),
        handoff("w12", "w24_all", "c1", "float32", False, data=2),
        hot("guided", 1, 24, 64, 8, 62, 97, guided=True, gocc="mask"), hot("guided", 2, 24, 200, 160, 63, 98, guided=True),
        hot("scaled", 2, 47, 165, 64, 64, 99, iscale=3, oscale=1, ds=True, gocc="mask"),
        hot("eval", 2, 40, 120, 64, 65, 100, iscale=2, oscale=2, evaluate=True),
        hot("sampled", 2, 32, 96, 64, 66, 104, evaluate=True, sample=dict(p=0.05, seed=9, source="gt", guided=False, outs=True)),
        metrics(3, 37, 53, 2, 105), metrics(3, 37, 53, 3, 106)])
    # 1. the resize tables: reused, rebuilt for another shape, rebuilt after calls that may have moved WS_SCALE_TAB
    A = hot("scaled", 2, 45, 170, 64, 21, 101, iscale=2, oscale=1, ds=True, gocc="heuristic")
    A2 = hot("scaled", 3, 47, 165, 64, 22, 102, iscale=3, oscale=2, ds=True, guided=True)
    h1 = handoff("w16_d24", "w65", "odd_pad", "float32", True)
    grow1 = dict(kind="fused", B=3, H=64, W=330, D=128, gocc="heuristic", rsgm=dict(pen(), subpixel=0), vpp=dict(), seed=23, data=103)
    part("tables", [A, A, A2, A, h1, A, grow1, A])
    # 2. the three parities: each call reads the set it wrote, and the data differ from call to call
    f1 = dict(kind="fused", B=8, H=40, W=120, D=64, gocc="none", rsgm=pen(), vpp=dict(), seed=31, data=111)
    sc = hot("scaled", 8, 40, 240, 64, 32, 112, iscale=2, oscale=2, rsgm=pen(), ds=True)
    sm = hot("sampled", 8, 40, 240, 64, 33, 113, rsgm=pen(), iscale=2, oscale=2,      # (the sampled call that also resizes)
             sample=dict(p=0.05, seed=2 ** 32 - 2, source="src", guided=False, outs=True))
    f2 = dict(kind="fused", B=8, H=40, W=120, D=64, gocc="mask", rsgm=pen(), vpp=dict(), seed=34, data=114)
    part("parities", [f1, sc, sm, f2])
    # 2b. what the two sets are for: with few frames per call the next call's front stage -- its resize, its sampling -- runs next
    #     to this call's guided rows, which still read the scaled / sampled hints.  Two scaled guided calls and two sampled guided
    #     calls back to back, the data different each time -- behind a call heavy enough that the device is still busy with it
    #     when the host has queued them, so that the two kernels become ready together
    busy = dict(kind="fused", B=4, H=64, W=330, D=256, gocc="none", rsgm=pen(), vpp=dict(), seed=39, data=119)
    ga = hot("scaled", 3, 45, 170, 64, 35, 115, iscale=2, oscale=1, guided=True, ds=True, p_hints=0.2)
    gb = hot("scaled", 3, 45, 170, 64, 36, 116, iscale=2, oscale=1, guided=True, ds=True, p_hints=0.2)
    pa = hot("sampled", 3, 40, 136, 64, 37, 117, sample=dict(p=0.2, seed=71, source="src", guided=True, outs=True))
    pb = hot("sampled", 3, 40, 136, 64, 38, 118, sample=dict(p=0.2, seed=72, source="src", guided=True, outs=True))
    part("hazards", [busy, ga, gb, ga, busy, pa, pb, pa])
    # 3. WS_DSI, WS_GUIDED_MAP and WS_PATHS change hands
    g256 = hot("guided", 3, 24, 100, 256, 41, 121, guided=True, gocc="heuristic")
    st64 = stage(64, 24, 48, 3)
    gall = hot("guided", 2, 24, 100, 64, 42, 122, guided=True, p_hints=1.0)
    fbyte = dict(kind="fused", B=9, H=24, W=100, D=64, gocc="none", rsgm=pen(), vpp=dict(), seed=43, data=123)
    gnone = hot("guided", 1, 24, 100, 64, 44, 124, guided=True, p_hints=0.0)
    part("dsi", [g256, st64, gall, fbyte, gnone])
    # 4. WS_HANDOFF_H / _V between the hand-off kernels and the host entries' staging
    h2 = handoff("w16_d24", "w130", "c1", "bfloat16", True, data=1)
    hv = host("call", 3, 40, 120, 64, 51, 131, guided=True)
    csmall = corr((1, 2, 63, 17), 4, 4, "float32", True)
    hs = host("scaled", 2, 45, 130, 64, 52, 132, iscale=2, oscale=1, guided=True, gocc="heuristic")
    part("handoff", [h2, hv, csmall, hs, h2])
    # 5. the PNG offsets of two calls in flight; then more partial records than ever before, then fewer
    part("png", [decode("png", files="three_small"), decode("png", files="one_stored"), metrics(16, 64, 330, 1, 141),
                 hot("eval", 1, 32, 96, 64, 53, 142, evaluate=True, rsgm=dict(_RK, alpha=1.0))])     # (the last table but for alpha)
    # 6. the graph block: an evaluating anchor, the same pointers each time
    E = hot("eval", 2, 32, 96, 64, 11, 151, evaluate=True, role="anchor")
    Em = dict(E, role="other_metrics", shares="anchor", own_in=(), own_out=("metrics",))     # the anchor's pointers but for metrics_out
    Eg = dict(E, role="other_gt", shares="anchor", own_in=("gt",), own_out=(), data=152)     # the anchor's pointers but for gt
    bs = hot("sampled", 2, 32, 96, 64, 12, 153, role="between", sample=dict(p=0.05, seed=5, source="src", guided=True, outs=False))
    bc = hot("scaled", 2, 64, 192, 64, 13, 154, role="between", iscale=2, oscale=2)
    grow = dict(role="grow", kind="fused", B=5, H=64, W=330, D=256, gocc="heuristic", rsgm=dict(pen(), subpixel=0), vpp=dict(), seed=13, data=3)
    part("graph", [E, E, E, Em, E, Eg, E, bs, E, bc, E, grow, E, E])
    calls += tail
    # 7. the call across one round of the lock-step kernel, as an evaluating call
    H, W, D = _QUANTUM_SHAPE
    part("crossing", [hot("eval", 2 * quantum + 1, H, W, D, 15, 5, evaluate=True, rsgm=pen())])
    specs = []
    for c in calls:
        if not any(c is x for x in specs):
            specs.append(c)
    order = [next(i for i, x in enumerate(specs) if x is c) for c in calls]
    return specs, order, marks


def expected_replays(order, specs, grew, first, last):
    """Graph replays of positions first..last of the order (all of them hot-path calls), from the rule of vppx_set_graph_mode:
    a call is served by the graph when its key -- the call itself, the workspace generation -- is the captured one and the
    penalty table is still its own; the second of two identical calls in a row is captured and launched; grew[p]: the workspace
    grew during position p (another generation).  Nothing before `first` has this block's keys."""
    gkey = lastkey = lut = None
    gen, out = 0, []
    for p in range(first, last + 1):
        i = order[p]
        pen = tuple(sorted((k, v) for k, v in specs[i]["rsgm"].items() if k in ("p2min", "gamma", "alpha")))
        key = (i, gen)
        if lut == pen and gkey == key:
            out.append(1)
        elif lut == pen and lastkey == key:
            gkey = key
            out.append(1)
        else:
            gen += int(grew[p])
            lastkey, lut = (i, gen), pen
            out.append(0)
    return out
