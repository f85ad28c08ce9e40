"""GPU: the timing helpers and stage timing, which every kernel figure of the benchmark passes through.

vppx_time_aggregate / _part RE-LAUNCH the last call's aggregation outside the call (on the images, penalties and geometry it
left in the context), vppx_agg_kernel_ms / vppx_we_kernel_ms read event rings every launch enters, stage timing switches the
hot path to its unpipelined, unsplit-over-streams, graph-less branches.  Held here:
  A. they disturb nothing: every output of every call after a helper equals the same call on a fresh engine, bit for bit;
  B. a helper launches what the call launched (vppx_timing_last_routes), a part only its kind of launch, and where that
     cannot be (the eight-path layout has no parts, a guided call's rows are not the helper's to read) it refuses first;
  C. the rings count launches: one per part of a call, one per helper iteration, none per graph replay, at most 64;
  D. nesting: an event pair that lies inside another on one stream reads no more than it, up to the clock's granularity,
     which the test measures itself (200 back-to-back pairs on an idle stream, the largest reading);
  E. stage timing on a call in parts: the same results, the same nesting, and no mark lost however many parts;
  F. after vppx_aggregate_img on the same context the helper restores its penalty table, or refuses where the gray image
     it would read has been overwritten or moved.
No ratio between two timed runs is asserted anywhere: toy sizes measure overheads, and the device is shared."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import _sequence_plan as P
import test_gpu_routes as TR

pytestmark = pytest.mark.gpu

E_INVALID_ARG, E_UNSUPPORTED = -1, -10
U16 = dict(P._RK, **TR._pen(232))          # 24 + P2max > 255: u16 path volumes
QH, QW, QD = P._QUANTUM_SHAPE
# VppxVppParams with their defaults written out (the referee wants every field it maps) and the maxDistance scan, which draws no
# random numbers
MAXDIST = dict(method=1, wsize=3, direction=1, c=0.4, uniform_color=0, c_occ=0.0, discard_occluded=0, interpolate=1)
WSUM_ENV = dict(VPPX_VERT=3, VPPX_VARIANT="wsum")     # as tests/test_gpu_wsum.py makes its engine


def _specs(quantum):
    """The smallest call that reaches each layout (the routes table of tests/test_gpu_routes.py is the source)."""
    return dict(
        eight=P.hot("eval", 2, 24, 112, 64, 3, 201, evaluate=True, gocc="heuristic"),
        eight_u16=P.hot("eval", 2, 24, 112, 64, 4, 202, evaluate=True, rsgm=dict(U16)),
        fused=P.hot("eval", 8, 24, 128, 128, 5, 203, evaluate=True, gocc="heuristic"),
        wsum=P.hot("eval", 3, 24, 208, 192, 6, 204, evaluate=True),
        quantum=P.hot("eval", quantum + 1, QH, QW, QD, 7, 205, evaluate=True),
        guided=P.hot("guided", 3, 24, 112, 64, 8, 206, guided=True, gocc="mask"),
        maxdist=P.hot("eval", 2, 24, 112, 64, 10, 209, evaluate=True, vpp=dict(MAXDIST)),
        sampled=P.hot("sampled", 3, 24, 112, 64, 9, 208, sample=dict(p=0.05, seed=5, source="src", guided=False, outs=True)),
    )


# what a layout's aggregation must be named, and what a helper does on it
EIGHT = lambda r: r.startswith("paths<") and r.endswith("dirs=ff>")
PART1 = lambda r: r.startswith("we12<") or (r.startswith("paths<") and (r.endswith("dirs=11>") or r.endswith("dirs=10>")))
PART2 = lambda r: r.startswith("vert3<") or r.startswith("vert4<")
AGG = lambda r: EIGHT(r) or PART1(r) or PART2(r)

_STATE = {}


def _quantum():
    if "quantum" not in _STATE:
        probe = P._env_engine()
        _STATE["quantum"] = probe.batch_quantum(QH, QW, QD)
        probe.ctx.close()
        assert _STATE["quantum"] >= 8, _STATE["quantum"]
    return _STATE["quantum"]


def _spec(name):
    if "specs" not in _STATE:
        _STATE["specs"] = _specs(_quantum())
        _STATE["data"] = {}
    if name not in _STATE["data"]:
        _STATE["data"][name] = P.plan_data([_STATE["specs"][name]])[0]
    return _STATE["specs"][name], _STATE["data"][name]


def _fresh(name, env=()):
    """The call on a fresh engine of this environment: (outputs on the host, route list, layout, pixels per wave, parts),
    computed once and left unchanged; held to the feature's own referee once per shape."""
    import torch
    key = ("ref", name, tuple(sorted(dict(env).items())))
    if key not in _STATE:
        s, d = _spec(name)
        eng = P._env_engine(**dict(env))
        try:
            t, bufs = P.plan_tensors(eng, [s], [d], 0, {})
            out = P.run(eng, s, d, t, bufs)
            torch.cuda.synchronize()
            eng.status()
            ref = {k: v.cpu() for k, v in out.items()}
            _STATE[key] = (ref, eng.last_routes(), eng.uses_vert(), eng.fused_pixels_per_wave(), eng.last_call_parts())
        finally:
            eng.ctx.close()
        if ("refereed", name) not in _STATE:
            P.referee(s, d, {k: P.host_array(v) for k, v in ref.items()})
            _STATE[("refereed", name)] = True
    return _STATE[key]


def _bits(x):
    """A tensor as integers of its own width: NaN cells compare by their bits (as tests/test_gpu_sequence_all.py)."""
    import torch
    view = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16}.get(x.dtype)
    return x.contiguous().view(view) if view is not None else x


def _same(got, ref, what):
    import torch
    assert got.keys() == ref.keys(), what
    for k, w in ref.items():
        g = got[k].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        assert torch.equal(_bits(g), _bits(w)), (what, k, int((_bits(g) != _bits(w)).sum()))


class Runner:
    """One engine, the device tensors of the calls it makes (the same pointers every time a call recurs)."""

    def __init__(self, env=(), pipelined=False, graph=False):
        import torch
        self.torch, self.env, self.pipelined, self.graph = torch, dict(env), pipelined, graph
        self.eng = P._env_engine(**self.env)
        self.side = torch.cuda.Stream(device=self.eng.device) if graph else None
        self.tens, self.ready = {}, None
        if pipelined:
            self.eng.set_pipeline(True)
        if graph:
            self.eng.set_graph_mode(True)

    def stream(self):
        return self.torch.cuda.stream(self.side) if self.graph else contextlib.nullcontext()

    def prepare(self, *names):
        with self.stream():
            for n in names:
                s, d = _spec(n)
                self.tens[n] = P.plan_tensors(self.eng, [s], [d], 0, {})
            self.torch.cuda.current_stream(self.eng.device).synchronize()
            if self.pipelined:      # every input exists behind this event: front stages may start next to the call before
                self.ready = self.torch.cuda.Event()
                self.ready.record()

    def call(self, name, check=True):
        s, d = _spec(name)
        with self.stream():
            out = P.run(self.eng, s, d, *self.tens[name], ready=self.ready)
            if not self.pipelined and not self.graph:
                self.eng.synchronize()
        if check:
            self.torch.cuda.synchronize()
            self.eng.status()
            _same(out, _fresh(name, self.env)[0], (name, self.env))
        return out

    def close(self):
        if self.graph:
            self.eng.set_graph_mode(False)
        self.torch.cuda.synchronize()
        self.eng.ctx.close()


def _refused(eng, fn, code, word):
    """The helper `fn(ms pointer)` refuses with `code` and a message that holds `word`, leaves *ms_out alone and launches
    nothing: no name in vppx_timing_last_routes, no launch in either ring."""
    from vppstereo_amd import _lib
    a0, w0 = eng.agg_kernel_ms(64)[1], eng.we_kernel_ms(64)[1]
    ms = C.c_float(-7.0)
    rc = fn(C.byref(ms))
    msg = eng.lib.vppx_last_error().decode()
    assert rc == code and word in msg, (rc, msg)
    assert ms.value == -7.0
    assert eng.timing_last_routes() == [] and (eng.agg_kernel_ms(64)[1], eng.we_kernel_ms(64)[1]) == (a0, w0)
    assert _lib.ERR_NAMES[rc]


def _helpers(eng, kind):
    """Steps 2 to 4 of the sequence: every helper that applies to the layout, the refusals where none does."""
    h, lib = eng.ctx.handle, eng.lib
    before = (eng.uses_vert(), eng.fused_pixels_per_wave(), eng.last_call_parts(), eng.last_routes())
    if kind == "guided":
        _refused(eng, lambda ms: lib.vppx_time_aggregate(h, 3, ms), E_UNSUPPORTED, "guided")
        _refused(eng, lambda ms: lib.vppx_time_aggregate_part(h, 2, 1, ms), E_UNSUPPORTED, "guided")
    else:
        assert eng.time_aggregate(3) > 0
        if kind == "eight":
            for part in (1, 2):
                _refused(eng, lambda ms: lib.vppx_time_aggregate_part(h, 2, part, ms), E_UNSUPPORTED, "eight-path")
        else:
            assert eng.time_aggregate_part(1, 2) > 0 and eng.time_aggregate_part(2, 2) > 0
    eng.agg_kernel_ms(4)
    eng.we_kernel_ms(4)
    eng.status()
    assert (eng.uses_vert(), eng.fused_pixels_per_wave(), eng.last_call_parts(), eng.last_routes()) == before


def _kind(name, env):
    if name == "guided":
        return "guided"
    return "fused" if _fresh(name, env)[2] == 3 else "eight"


# Every configuration of _sequence_plan.CONFIGS, VPPX_CHUNK=3 and the wsum engine, each with every layout it can reach.  What a
# configuration cannot reach, and so does not list:
#   - "wsum" (the W + sum + WTA route) needs the engine of tests/test_gpu_wsum.py: it is the configurations wsum*, which reach
#     nothing else that the others do not;
#   - "sampled" differs from the other eight-path calls only in its front stage, which matters where front stages run ahead
#     (pipelined: the two sets of maps);
#   - under VPPX_SUBSTREAMS=2 and VPPX_VERT=0 no call is fused (the children stay on the line-parallel kernel): the fused and
#     quantum SHAPES run there, in the eight-path layout;
#   - under VPPX_CHUNK=3 no part holds more than 3 frames, so W/E never runs next to an under-filled launch of a batch above
#     one quantum: the quantum shape runs there as parts of the fused layout.
_BY = {c[0]: c for c in P.CONFIGS}
_EIGHTS = ["eight", "eight_u16", "guided", "maxdist"]
SEQUENCES = [
    ("default", _EIGHTS + ["fused", "quantum"]),
    ("pipelined", _EIGHTS + ["fused", "quantum", "sampled"]),
    ("graph", _EIGHTS + ["fused", "quantum"]),
    ("substreams", _EIGHTS + ["fused", "quantum"]),
    ("vert0", _EIGHTS + ["fused", "quantum"]),
    ("chunk", _EIGHTS + ["fused", "quantum"]),
    ("wsum", ["wsum"]),
    ("wsum_pipelined", ["wsum"]),
    ("wsum_graph", ["wsum"]),
]
CASES = [(c, x) for c, xs in SEQUENCES for x in xs]


def _config(name):
    if name == "chunk":
        return dict(VPPX_CHUNK=3), False, False
    if name == "after":         # W/E never next to an under-filled lock-step launch: always behind it, on the launch stream
        return dict(VPPX_VARIANT="we_after"), False, False
    if name == "wsum_after":
        return dict(WSUM_ENV, VPPX_VARIANT="wsum,we_after"), False, False
    if name.startswith("wsum"):
        return dict(WSUM_ENV), name.endswith("pipelined"), name.endswith("graph")
    return _BY[name][1], _BY[name][2], _BY[name][3]


def _replay_model(order, specs, grew):
    """_sequence_plan.expected_replays' rule over a sequence that may hold a stage-timed call, order[p] = (spec, staged): such a
    call runs eagerly beside the graph -- it is no replay, uploads its own penalty table where another one lies, may grow the
    workspace, and neither becomes the key the next call is compared with nor destroys the graph (include/vppx.h)."""
    gkey = lastkey = lut = None
    gen, out = 0, []
    for (i, staged), g in zip(order, grew):
        pen = tuple(sorted((k, v) for k, v in specs[i]["rsgm"].items() if k in ("p2min", "gamma", "alpha")))
        key = (i, gen)
        if staged:
            gen += int(g)
            lut = pen
            out.append(0)
        elif lut == pen and gkey == key:
            out.append(1)
        elif lut == pen and lastkey == key:
            gkey = key
            out.append(1)
        else:
            gen += int(g)
            lastkey, lut = (i, gen), pen
            out.append(0)
    return out


def _sequence(config, x, y, helpers):
    """Steps 1 to 12 on one engine, every call checked against the fresh engine's; without `helpers`, the same calls with
    steps 2 to 4 left out.  What was recorded per call: (order, graph replays, workspace grew, front sets)."""
    env, pipelined, graph = _config(config)
    kind = _kind(x, env)
    r = Runner(env, pipelined, graph)
    eng = r.eng
    order, replays, grew, sets = [], [], [], []
    ws = lambda: int(eng.lib.vppx_workspace_bytes(eng.ctx.handle))

    def call(n, staged=False):
        r0, w0 = eng.graph_replays(), ws()
        r.call(n)
        order.append((0 if n == x else 1, staged))
        replays.append(eng.graph_replays() - r0)
        grew.append(ws() > w0)
        if config not in ("substreams",) and not staged:       # (the children keep lists of their own)
            assert eng.last_routes() == _fresh(n, env)[1], (n, eng.last_routes())
            assert eng.last_call_parts() == _fresh(n, env)[4]
        sets.append(eng.last_front_sets())

    try:
        r.prepare(x, y)
        call(x)
        if graph:
            call(x)         # captured and launched
            call(x)         # replayed
        if helpers:
            r0 = eng.graph_replays()
            with r.stream():
                _helpers(eng, kind)
            assert eng.graph_replays() == r0
        call(x)
        call(y)
        with r.stream():
            eng.enable_stage_timing(True)
        call(x, staged=True)
        with r.stream():
            st = eng.stage_ms()
        assert eng.stage_marks() >= (8 if x == "maxdist" else 9) and all(v >= 0 for v in st.values()), st     # (no mark of vpp_rand)
        assert st["aggregate_8paths"] > 0 and st["post"] > 0, st
        eng.enable_stage_timing(False)
        assert eng.stage_marks() == 0
        call(x)
        call(y)
    finally:
        r.close()
    return order, replays, grew, sets


@pytest.mark.parametrize("config, x", CASES, ids=[f"{c}-{x}" for c, x in CASES])
def test_helpers_and_stage_timing_disturb_nothing(config, x):
    """A. X, the helpers, X, Y, stage timing on, X, its stage times, off, X, Y on one engine: every output equals the fresh
    engine's, the status stays clean, the layout queries are what they were before a helper, a pipelined context starts every
    front stage on the set it takes in the same sequence without helpers, the graph replays fall where the key says -- before,
    at and behind the stage-timed call -- and a helper costs none."""
    env, pipelined, graph = _config(config)
    y = "eight" if x in ("fused", "wsum", "quantum") else "fused"
    fx, fy = _fresh(x, env), _fresh(y, env)
    B = _spec(x)[0]["B"]
    if config == "default":
        want = dict(eight=0, eight_u16=0, fused=3, quantum=3, guided=0, maxdist=0)[x]
        assert fx[2] == want, (x, fx[2])
    if config == "chunk":           # (a call of up to 3 frames is one part)
        assert (fx[4] == 1) if B <= 3 else (fx[4] >= 2), (B, fx[4])
        if x == "fused":
            assert fx[4] == 2, fx[4]
    if config in ("substreams", "vert0"):
        assert fx[2] == 0
    order, replays, grew, sets = _sequence(config, x, y, True)
    if pipelined:
        plain = _sequence(config, x, y, False)
        assert plain[0] == order and sets == plain[3], (sets, plain[3])
        if x == "sampled":      # ... which, for the sampling calls, is the alternation between the two sets of maps
            mine = [st[1] for st, (o, staged) in zip(sets, order) if o == 0 and not staged]
            assert mine == [k % 2 for k in range(len(mine))] and len(mine) == 3, sets
    if graph:
        specs = [dict(rsgm=_spec(x)[0]["rsgm"]), dict(rsgm=_spec(y)[0]["rsgm"])]
        first = [p for p, (o, staged) in enumerate(order) if staged][0]
        head = [o for o, _ in order[:first]]
        want = _replay_model(order, specs, grew)
        assert want[:first] == P.expected_replays(head, specs, grew[:first], 0, first - 1), want
        assert replays == want, (replays, want, grew)
        assert replays[:3] == [0, 1, 1] and replays[3] == 1, replays      # the helpers between two identical calls cost no replay
        assert replays[first] == 0
        if not any(grew[first - 1:]):       # nothing moved: the graph of X outlives the stage-timed call
            assert replays[first + 1] == 1, (replays, grew)
    else:
        assert not any(replays), replays


@pytest.mark.parametrize("config, x", [("default", "eight"), ("default", "eight_u16"), ("default", "fused"), ("default", "quantum"),
                                       ("default", "guided"), ("wsum", "wsum"), ("chunk", "fused"), ("substreams", "fused")],
                         ids=lambda v: v)
def test_a_helper_launches_what_the_call_launched(config, x):
    """B. vppx_last_routes after a helper is the call's list; vppx_timing_last_routes names the call's aggregation kernels for
    the whole stage, a subset of the W/E names for part 1, of the lock-step names for part 2, and the two parts together are the
    whole; the eight-path layout has no parts and a guided call nothing to re-launch: both refuse before they launch."""
    env, _, _ = _config(config)
    kind = _kind(x, env)
    r = Runner(env)
    eng = r.eng
    h, lib = eng.ctx.handle, eng.lib
    try:
        r.prepare(x)
        r.call(x)
        routes = eng.last_routes()
        if config == "substreams":
            assert routes == []         # (not merged: the helper's own list is child 0's)
        if kind == "guided":
            _refused(eng, lambda ms: lib.vppx_time_aggregate(h, 2, ms), E_UNSUPPORTED, "guided")
            assert eng.last_routes() == routes and eng.uses_vert() == 0
            return
        assert eng.time_aggregate(2) > 0
        whole = eng.timing_last_routes()
        assert eng.last_routes() == routes
        assert whole and all(AGG(n) for n in whole), whole
        if config != "substreams":
            assert whole == [n for n in routes if AGG(n)], (whole, routes)
        if kind == "eight":
            assert len(whole) == 1 and EIGHT(whole[0]), whole
            for part in (1, 2):
                _refused(eng, lambda ms: lib.vppx_time_aggregate_part(h, 2, part, ms), E_UNSUPPORTED, "eight-path")
                assert eng.last_routes() == routes
            return
        parts = {}
        for part, ok in ((1, PART1), (2, PART2)):
            r.call(x)       # a fresh copy of the call
            assert eng.time_aggregate_part(part, 2) > 0
            parts[part] = eng.timing_last_routes()
            assert eng.last_routes() == routes, (part, eng.last_routes(), routes)
            assert parts[part] and all(ok(n) for n in parts[part]), (part, parts[part])
        assert set(parts[1]) | set(parts[2]) == set(whole) and not set(parts[1]) & set(parts[2]), (parts, whole)
        assert eng.fused_pixels_per_wave() == _fresh(x, env)[3]
        if x == "wsum":
            assert "wsum<12>" in routes
        _refused(eng, lambda ms: lib.vppx_time_aggregate_part(h, 2, 3, ms), E_INVALID_ARG, "part must be 1 or 2")
        r.call(x)
    finally:
        r.close()


def _counts(eng):
    return eng.agg_kernel_ms(64)[1], eng.we_kernel_ms(64)[1]


@pytest.mark.parametrize("config, x, per_call", [("default", "eight", (1, 0)), ("default", "fused", (1, 1)), ("default", "quantum", (1, 1)),
                                                 ("wsum", "wsum", (1, 1)), ("chunk", "fused", (2, 2)), ("substreams", "fused", (1, 0))],
                         ids=lambda v: str(v))
def test_the_rings_count_launches(config, x, per_call):
    """C. K = 3 calls after a reset: one aggregation launch per part of a call (child 0's, under sub-streams), one W/E launch
    per part in the fused layout -- also where that launch makes E only -- and none in the eight-path layout; last_n bounds
    the answer; a helper adds its iterations to the ring of what it launches, and to no other."""
    env, _, _ = _config(config)
    r = Runner(env)
    eng = r.eng
    K = 3
    try:
        r.prepare(x)
        r.call(x)
        eng.agg_kernel_ms(0)
        eng.we_kernel_ms(0)
        assert _counts(eng) == (0, 0)
        for _ in range(K):
            r.call(x, check=False)
        r.torch.cuda.synchronize()
        eng.status()
        if config == "chunk":
            assert eng.last_call_parts() == 2
        assert _counts(eng) == (K * per_call[0], K * per_call[1]), _counts(eng)
        assert eng.agg_kernel_ms(2)[1] == 2 and eng.agg_kernel_ms(2)[0] > 0
        B = _spec(x)[0]["B"]
        assert eng.time_aggregate_frames() == dict(chunk=3, substreams=B // 2).get(config, B)
        a0, w0 = _counts(eng)
        eng.time_aggregate(5)
        fused = per_call[1] > 0
        assert _counts(eng) == (a0 + 5, w0 + (5 if fused else 0)), _counts(eng)
        if fused:
            a0, w0 = _counts(eng)
            eng.time_aggregate_part(1, 5)
            assert _counts(eng) == (a0, w0 + 5), _counts(eng)
            eng.time_aggregate_part(2, 5)
            assert _counts(eng) == (a0 + 5, w0 + 5), _counts(eng)
        if x == "eight" and config == "default":
            eng.agg_kernel_ms(0)
            eng.time_aggregate(70)
            assert eng.agg_kernel_ms(100)[1] == 64
    finally:
        r.close()


def test_a_graph_replay_adds_nothing_to_the_rings():
    """C. Event records stay out of a captured graph: of three identical calls in graph mode only the first, eager one counts."""
    r = Runner((), graph=True)
    eng = r.eng
    try:
        r.prepare("fused")
        with r.stream():
            eng.agg_kernel_ms(0)
            eng.we_kernel_ms(0)
        n0 = eng.graph_replays()
        for _ in range(3):
            r.call("fused")
        assert eng.graph_replays() - n0 == 2
        assert _counts(eng) == (1, 1), _counts(eng)
    finally:
        r.close()


def test_bad_arguments_and_a_helper_before_any_call_launch_nothing():
    """C. iters = 0, a NULL ms_out, a helper on a context that has run no rSGM call: VPPX_E_INVALID_ARG, nothing launched."""
    r = Runner()
    eng = r.eng
    h, lib = eng.ctx.handle, eng.lib
    try:
        eng._bind_stream()
        _refused(eng, lambda ms: lib.vppx_time_aggregate(h, 3, ms), E_INVALID_ARG, "call vppx_rsgm_dev first")
        _refused(eng, lambda ms: lib.vppx_time_aggregate_part(h, 3, 1, ms), E_INVALID_ARG, "call vppx_rsgm_dev first")
        assert eng.time_aggregate_frames() == 0
        r.prepare("eight")
        r.call("eight")
        _refused(eng, lambda ms: lib.vppx_time_aggregate(h, 0, ms), E_INVALID_ARG, "iters must be positive")
        _refused(eng, lambda ms: lib.vppx_time_aggregate_part(h, -1, 1, ms), E_INVALID_ARG, "iters must be positive")
        _refused(eng, lambda ms: lib.vppx_time_aggregate(h, 3, None), E_INVALID_ARG, "ms_out is NULL")
        r.call("eight")
    finally:
        r.close()


def _granularity(torch, dev):
    """The largest of 200 back-to-back event pairs on an idle stream: what one pair may read with nothing between its events."""
    if "gran" not in _STATE:
        torch.cuda.synchronize()
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(200)]
        for a, b in pairs:
            a.record()
            b.record()
        torch.cuda.synchronize()
        _STATE["gran"] = max(a.elapsed_time(b) for a, b in pairs)
        print(f"\n[timing] hipEventElapsedTime granularity, largest of 200 empty pairs: {_STATE['gran'] * 1000:.2f} us")
    return _STATE["gran"]


NEVER = {"occlusion_heuristic": lambda s, routes: s["gocc"] != "heuristic", "wta_right": lambda s, routes: "wta_right_t" not in routes,
         "vpp_rand": lambda s, routes: s["vpp"].get("method") == 1}
RAN = ("vpp_compact", "vpp_apply", "pad_gray", "aggregate_8paths", "sum_wta_left", "median_interp", "post")


def _staged_call(r, x, env):
    """Call X with stage timing on inside one pair of torch events on the engine's stream: (stage times, outer ms, marks)."""
    torch, eng = r.torch, r.eng
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.enable_stage_timing(True)
    e0.record()
    got = r.call(x, check=False)
    e1.record()
    torch.cuda.synchronize()
    eng.status()
    _same(got, _fresh(x, env)[0], (x, "stage timing"))
    st, marks = eng.stage_ms(), eng.stage_marks()
    return st, e0.elapsed_time(e1), marks


def _nesting(st, outer, marks, gran, s, routes):
    assert all(v >= 0 for v in st.values()), st
    assert sum(st.values()) <= outer + (marks + 1) * gran, (st, outer, gran)
    for k in RAN:
        assert st[k] > 0, (k, st)
    for k, never in NEVER.items():
        if never(s, routes):
            assert st[k] == 0.0, (k, st)
        else:
            assert st[k] > 0, (k, st)


@pytest.mark.parametrize("config, x", [("default", "eight"), ("default", "maxdist"), ("default", "fused"), ("after", "fused"), ("default", "quantum"),
                                       ("wsum", "wsum"), ("wsum_after", "wsum")], ids=lambda v: v)
def test_inner_intervals_fit_into_outer_ones(config, x):
    """D. Stream order, not performance: the stages of a call sum to no more than a pair around the call; the ring's pair
    around the aggregation launch(es) lies inside the aggregation stage; the rings' pairs of five helper iterations lie inside
    the helper's own pair.  Each comparison allows the measured granularity once per event pair that enters it.  A batch below
    one round of the lock-step kernel -- every fused shape here -- runs W/E on the side stream NEXT to that launch, behind a
    join the stage's mark waits for: there each launch alone fits into the stage; under VPPX_VARIANT=we_after W/E runs behind
    the lock-step launch on the launch stream, and there the two together do."""
    env, _, _ = _config(config)
    r = Runner(env)
    eng = r.eng
    try:
        r.prepare(x)
        r.call(x)
        gran = _granularity(r.torch, eng.device)
        assert 0 <= gran < 1.0, gran        # (a millisecond of "nothing" would make every bound below empty)
        s, routes = _spec(x)[0], _fresh(x, env)[1]
        fused = _fresh(x, env)[2] == 3
        behind = config in ("after", "wsum_after")
        eng.agg_kernel_ms(0)
        eng.we_kernel_ms(0)
        st, outer, marks = _staged_call(r, x, env)
        print(f"[timing] {config}-{x}: stages {st}, outer {outer:.3f} ms, {marks} marks")
        _nesting(st, outer, marks, gran, s, routes)
        a, na = eng.agg_kernel_ms(1)
        w, nw = eng.we_kernel_ms(1)
        assert na == 1 and nw == (1 if fused else 0)
        agg = st["aggregate_8paths"]
        assert 0 < a <= agg + 2 * gran, (a, agg)
        if fused:
            assert 0 < w <= agg + 2 * gran, (w, agg)
            if behind:                  # one after the other inside the stage
                assert a + w <= agg + 3 * gran, (a, w, agg)
        eng.enable_stage_timing(False)
        t = eng.time_aggregate(5)
        a, na = eng.agg_kernel_ms(5)
        w, nw = eng.we_kernel_ms(5)
        assert t > 0 and a > 0 and na == 5 and nw == (5 if fused else 0)
        if not fused:
            assert 5 * a <= 5 * t + 6 * gran, (a, t)
        elif behind:
            assert w > 0 and 5 * (a + w) <= 5 * t + 11 * gran, (a, w, t)
        else:                           # W/E beside the under-filled launch: each alone
            assert w > 0 and 5 * a <= 5 * t + 6 * gran and 5 * w <= 5 * t + 6 * gran, (a, w, t)
        r.call(x)
    finally:
        r.close()


def test_stage_timing_on_a_call_in_parts():
    """E. VPPX_CHUNK=3, 8 frames: the parts' marks follow one another, the outputs are the unsplit fresh engine's, the stages
    nest in one pair around the whole call, and there are as many marks as two calls of one part each make."""
    env = dict(VPPX_CHUNK=3)
    r = Runner(env)
    eng = r.eng
    try:
        r.prepare("fused")
        r.call("fused")
        gran = _granularity(r.torch, eng.device)
        st, outer, marks = _staged_call(r, "fused", ())        # against the UNSPLIT fresh engine
        assert eng.last_call_parts() == 2
        _nesting(st, outer, marks, gran, _spec("fused")[0], _fresh("fused", env)[1])
        assert marks in (20, 21, 22), marks         # 10 or 11 per part with the heuristic
        eng.enable_stage_timing(False)
        r.call("fused")
    finally:
        r.close()


def test_no_stage_mark_is_lost_in_many_parts():
    """E. VPPX_CHUNK=1, 12 frames of 16 x 48, D = 64: 12 parts of 9 marks each (no heuristic, no fallback; 10 or 11 with
    them), more than the 96 slots the table once had, which dropped everything behind the 96th without a sign.
    The outputs are the unsplit call's, and the marks are 12 times those of the same call on one frame."""
    import torch
    s12 = P.hot("guided", 12, 16, 48, 64, 9, 207)
    s1 = dict(s12, B=1)
    d12 = P.plan_data([s12])[0]
    d1 = {k: np.ascontiguousarray(v[:1]) for k, v in d12.items()}
    ref_eng = P._env_engine()
    try:
        t, bufs = P.plan_tensors(ref_eng, [s12], [d12], 0, {})
        ref = {k: v.cpu() for k, v in P.run(ref_eng, s12, d12, t, bufs).items()}
        torch.cuda.synchronize()
        assert ref_eng.last_call_parts() == 1
    finally:
        ref_eng.ctx.close()
    P.referee(s12, d12, {k: P.host_array(v) for k, v in ref.items()})
    eng = P._env_engine(VPPX_CHUNK=1)
    try:
        eng.enable_stage_timing(True)
        t1, b1 = P.plan_tensors(eng, [s1], [d1], 0, {})
        P.run(eng, s1, d1, t1, b1)
        torch.cuda.synchronize()
        per_part = eng.stage_marks()
        assert per_part in (9, 10, 11), per_part
        t, bufs = P.plan_tensors(eng, [s12], [d12], 0, {})
        got = P.run(eng, s12, d12, t, bufs)
        torch.cuda.synchronize()
        eng.status()
        assert eng.last_call_parts() == 12
        _same(got, ref, "12 parts")
        assert eng.stage_marks() == 12 * per_part > 96, eng.stage_marks()
        st = eng.stage_ms()
        assert all(st[k] > 0 for k in RAN), st
        eng.enable_stage_timing(False)
    finally:
        torch.cuda.synchronize()
        eng.ctx.close()


def _aggregate_img(eng, H, W, D, channels, seed):
    """vppx_aggregate_img (what pyrSGM.aggregate_SSE calls) on THIS engine's context, with penalties far from the call's."""
    from vppstereo_amd import _lib
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, channels) if channels == 3 else (H, W), dtype=np.uint8)
    dsi = rng.integers(0, 25, (H, W, D)).astype(np.uint16)
    S = np.zeros_like(dsi)
    eng._bind_stream()
    _lib.check(eng.lib.vppx_aggregate_img(eng.ctx.handle, _lib.np_ptr(img), channels, _lib.np_ptr(dsi), _lib.np_ptr(S), W, H, D, 3, 90, 2.0, 200))
    assert S.any()


def test_helper_after_the_stage_api_still_runs_and_disturbs_no_later_call():
    """F1. aggregate_SSE with other penalties on a smaller frame overwrites the device's penalty table and moves no buffer: the
    helper still runs and re-launches the call's kernels, and the calls behind it are the fresh engine's.  (Whether the helper
    uploaded the call's table again cannot be seen here -- a later call uploads its own where the table is marked foreign; the
    next test sees it.)"""
    r = Runner()
    eng = r.eng
    try:
        r.prepare("fused", "eight")
        r.call("fused")
        routes = eng.last_routes()
        _aggregate_img(eng, 16, 64, 32, 1, 1)
        assert eng.time_aggregate_frames() == 8
        assert eng.time_aggregate(2) > 0
        assert eng.timing_last_routes() == [n for n in routes if AGG(n)]
        assert eng.time_aggregate_part(1, 2) > 0 and eng.time_aggregate_part(2, 2) > 0
        eng.status()
        r.call("fused")
        r.call("eight")
    finally:
        r.close()


def test_helper_after_the_stage_api_uploads_the_calls_penalty_table_again():
    """F1, the upload made visible.  A captured graph holds no upload of the penalty table, so vppx_set_graph_mode replays it
    only while the table on the device is marked as the call's.  aggregate_SSE overwrites the table and marks it foreign: the
    identical call behind it is no replay (the control).  With a helper in between it is one -- the helper marked the table as
    the call's -- and its outputs are the fresh engine's, which they are only if the helper also uploaded it: the replay
    uploads nothing, and the other table's penalties (P2min 90, gamma 200, alpha 2 against 15, 40, 0.5) give other disparities."""
    r = Runner((), graph=True)
    eng = r.eng
    ws = lambda: int(eng.lib.vppx_workspace_bytes(eng.ctx.handle))
    try:
        r.prepare("fused")
        with r.stream():
            _aggregate_img(eng, 16, 64, 32, 1, 1)       # its staging buffers exist from here on: the later ones move nothing
        n0 = eng.graph_replays()
        for _ in range(3):
            r.call("fused")
        assert eng.graph_replays() - n0 == 2
        w0, n0 = ws(), eng.graph_replays()
        with r.stream():
            _aggregate_img(eng, 16, 64, 32, 1, 1)
            assert eng.time_aggregate(2) > 0
        r.call("fused")
        assert ws() == w0 and eng.graph_replays() - n0 == 1
        with r.stream():                                # the control: no helper, no replay; the call uploads its table itself
            _aggregate_img(eng, 16, 64, 32, 1, 1)
        r.call("fused")
        assert ws() == w0 and eng.graph_replays() - n0 == 1
    finally:
        r.close()


def test_helper_after_a_colour_image_through_the_stage_api_refuses():
    """F2. aggregate_SSE with a 3-channel image converts it into the buffer the last call's gray image lies in, and a LARGER
    frame moves that buffer: the helper has nothing of the call left to read and says so before it launches anything."""
    r = Runner()
    eng = r.eng
    h, lib = eng.ctx.handle, eng.lib
    try:
        r.prepare("fused")
        r.call("fused")
        _aggregate_img(eng, 160, 256, 32, 3, 2)     # 40960 gray bytes: more than the call's 8 frames of 32 x 128 padded pixels
        _refused(eng, lambda ms: lib.vppx_time_aggregate(h, 2, ms), E_INVALID_ARG, "call vppx_rsgm_dev first")
        _refused(eng, lambda ms: lib.vppx_time_aggregate_part(h, 2, 2, ms), E_INVALID_ARG, "call vppx_rsgm_dev first")
        assert eng.time_aggregate_frames() == 0
        r.call("fused")
        assert eng.time_aggregate(2) > 0
    finally:
        r.close()
