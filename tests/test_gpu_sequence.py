"""GPU: one long-lived context through a seeded sequence of unlike calls.

Callers keep one context for thousands of calls (bench.py, FrameStream), and the library carries state from call to call:
workspace buffers that only grow, buffers cleared once when allocated, clears deferred to the pipelined front stage, launch
serials, the cached penalty table, the cached graph and its key, the sub-stream child contexts.  Every other GPU test builds a
fresh engine per case or repeats one geometry.  Here each configuration runs a whole plan -- fused calls, VPP + rSGM, the
occlusion heuristic alone, the post stage; batch sizes across the lock-step round, disparity ranges from 8 to 256, penalties
that keep the fused layout and penalties that force the eight-path / u16 volumes, masks and heuristic masks -- on ONE engine,
and every result must equal the same call on a fresh engine (which has no history) bit for bit.  Frames 0 and B - 1 of every
call are checked against the CPU oracle once per seed."""
import contextlib

import numpy as np
import pytest

import oracle
import synth

pytestmark = pytest.mark.gpu

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


def _plan(seed, quantum):
    """The calls of one sequence, in order (a spec that occurs twice is the SAME call: same tensors, same parameters)."""
    rng = np.random.default_rng(4242 + seed)
    anchor = dict(_ANCHOR)
    other_seed = dict(anchor, role=None, seed=12)            # another key, same workspace, same penalty table
    rk = _penalties(rng, "fused")
    rk.update(subpixel=1, uniqueness=0.95)
    other_pen = dict(anchor, role=None, rsgm=rk, data=2)     # another penalty table only
    grow = dict(role="grow", kind="fused", B=5, H=64, W=330, D=256, gocc="heuristic", rsgm=dict(_penalties(rng, "fused"), subpixel=0, uniqueness=0.95),
                vpp=dict(), seed=13, data=3)                 # the largest call so far: the workspace grows
    fused3 = dict(kind="fused", B=int(rng.choice([8, 9])), H=40, W=120, D=192, gocc=str(rng.choice(["none", "mask", "heuristic"])),
                  rsgm=dict(_penalties(rng, "fused"), subpixel=1, uniqueness=0.95), vpp=dict(), seed=14, data=4,
                  occ=dict(rx=9, ry=7, l=2.0, g=0.4375, th_conf=1.0, th_filter=0.1))
    H, W, D = _QUANTUM_SHAPE
    crossing = dict(kind="fused", B=2 * quantum + 1, H=H, W=W, D=D, gocc="none", rsgm=dict(_penalties(rng, "fused"), subpixel=1, uniqueness=0.95),
                    vpp=dict(), seed=15, data=5)
    calls = [_random_call(rng, True, "split"), _random_call(rng, True, "occ"), fused3,
             anchor, anchor, anchor, other_seed, anchor, other_pen, anchor, anchor, grow, anchor, anchor]
    calls += [_random_call(rng, False, "post")] + [_random_call(rng, False) for _ in range(int(rng.integers(1, 5)))]
    calls.append(crossing)
    specs = []
    for c in calls:
        if not any(c is s for s in specs):
            specs.append(c)
    order = [next(i for i, s in enumerate(specs) if s is c) for c in calls]
    return specs, order


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


def _run(eng, s, t, bufs):
    """One call of the plan on `eng` with the call's own device tensors `t` and output buffers `bufs`; returns its outputs
    (cloned on the current stream, so that a later occurrence of the same call may reuse the buffers)."""
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
                     vpp_kw=s["vpp"], rsgm_kw=rk, occ_out=bufs["occ"] if heur else None)
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
    import os
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


_PREPARED = {}


def _prepared(seed):
    """(specs, order, host data, reference outputs): each reference is the call on a fresh engine, closed afterwards."""
    if seed not in _PREPARED:
        import torch
        probe = _env_engine()
        quantum = probe.batch_quantum(*_QUANTUM_SHAPE)
        probe.ctx.close()
        assert quantum >= 8, quantum
        specs, order = _plan(seed, quantum)
        data = [_data(s) for s in specs]
        refs = []
        for s, d in zip(specs, data):
            eng = _env_engine()
            t, bufs = _tensors(eng, s, d)
            refs.append([x.cpu() for x in _run(eng, s, t, bufs)])
            torch.cuda.synchronize()
            eng.ctx.close()
        _PREPARED[seed] = (specs, order, data, refs)
    return _PREPARED[seed]


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
    v = s["vpp"]
    vk = dict(wsize=v["wsize"], left2right=bool(v["direction"]), blending=v["c"], uniform_color=bool(v["uniform_color"]), c_occ=v["c_occ"],
              discard_occ=bool(v["discard_occluded"]), interpolate=bool(v["interpolate"])) if v else {}
    oracle.init_rand(s["seed"] + f)
    lo, ro = oracle.vpp(d["left"][f], d["right"][f], d["hints"][f], g_occ=conf, **vk)
    rk = dict(s["rsgm"], dmax=s["D"])
    rk["subpixel"] = bool(rk["subpixel"])
    r = [oracle.compute_rsgm(d["left"][f], lo, ro, **rk), lo, ro]
    if s["gocc"] in ("heuristic", "params"):
        r.append(conf)
    return r


@pytest.mark.parametrize("seed", range(4))
def test_sequence_references_match_oracle(seed):
    """The fresh-engine references every configuration is held to: frames 0 and B - 1 of every call equal the CPU oracle."""
    specs, order, data, refs = _prepared(seed)
    assert 12 <= len(order) <= 20 and {s["kind"] for s in specs} == {"fused", "split", "occ", "post"}, [s["kind"] for s in specs]
    for i, (s, d, ref) in enumerate(zip(specs, data, refs)):
        for f in sorted({0, s["B"] - 1}):
            want = _oracle(s, d, f)
            assert len(want) == len(ref), (i, s["kind"])
            for k, (w, g) in enumerate(zip(want, ref)):
                assert np.array_equal(w, g[f].numpy()), (i, f, k, {x: s[x] for x in ("kind", "B", "H", "W", "D", "gocc")}, s["rsgm"])


# (name, environment, pipelined, graph mode)
_CONFIGS = [
    ("default", dict(), False, False),
    ("vert3", dict(VPPX_VERT=3), False, False),
    ("vert0", dict(VPPX_VERT=0), False, False),
    ("pipelined", dict(), True, False),
    ("substreams", dict(VPPX_SUBSTREAMS=2), False, False),
    ("graph", dict(), False, True),
]


@pytest.mark.parametrize("config", _CONFIGS, ids=[c[0] for c in _CONFIGS])
@pytest.mark.parametrize("seed", range(4))
def test_one_context_through_a_sequence_of_unlike_calls(seed, config):
    """One engine runs the whole plan (pipelined: with no synchronisation between calls; graph mode: on a side stream, the anchor
    call recurring after calls that change only the seed, only the penalty table, or grow the workspace); every output of every
    call equals the fresh-engine reference.  The paths are shown taken: the aggregation layout changes within the default and
    pipelined sequences, the call across the lock-step round runs in parts, graph replays happen after intervening calls."""
    import torch
    name, env, pipelined, graph = config
    specs, order, data, refs = _prepared(seed)
    eng = _env_engine(**env)
    side = torch.cuda.Stream(device=eng.device) if graph else None
    layouts, parts, replays, grew = set(), [], [], None
    got = []
    try:
        if pipelined:
            eng.set_pipeline(True)
        if graph:
            eng.set_graph_mode(True)
        ws = lambda: int(eng.lib.vppx_workspace_bytes(eng.ctx.handle))
        with torch.cuda.stream(side) if graph else contextlib.nullcontext():
            tens = [_tensors(eng, s, d) for s, d in zip(specs, data)]
            torch.cuda.current_stream(eng.device).synchronize()
            for pos, i in enumerate(order):
                s = specs[i]
                r0, w0 = eng.graph_replays(), ws()
                got.append(_run(eng, s, *tens[i]))
                if not pipelined and not graph:
                    eng.synchronize()
                if s["kind"] in ("fused", "split"):
                    layouts.add(eng.uses_vert())
                if s["kind"] == "fused":
                    parts.append(eng.last_call_parts())
                replays.append(eng.graph_replays() - r0)
                if s.get("role") == "grow":
                    grew = ws() > w0
            eng.synchronize()
        for pos, i in enumerate(order):
            for k, (g, w) in enumerate(zip(got[pos], refs[i])):
                assert torch.equal(g.cpu(), w), (name, pos, i, k, {x: specs[i][x] for x in ("kind", "B", "H", "W", "D", "gocc")},
                                                 int((g.cpu() != w).sum()))
        if name in ("default", "pipelined"):
            assert len(layouts) >= 2, layouts
        if name == "default":
            assert max(parts) > 1, parts
        if graph:
            role = [specs[i].get("role") for i in order]
            assert sum(replays) >= 3, replays
            # a replay of the anchor right behind another call (the one that changed neither the workspace nor the penalty table)
            assert any(replays[p] > 0 and role[p] == "anchor" and role[p - 1] != "anchor" for p in range(1, len(order))), (role, replays)
            # the growing call grew the workspace; the anchor behind it ran eagerly (another workspace generation), the next was
            # captured again and launched from the new graph
            pg = role.index("grow")
            assert grew and role[pg + 1:pg + 3] == ["anchor", "anchor"], (grew, role)
            assert replays[pg + 1] == 0 and replays[pg + 2] == 1, replays
    finally:
        if graph:
            eng.set_graph_mode(False)
        torch.cuda.synchronize()
        eng.ctx.close()
