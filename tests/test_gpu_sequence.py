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

# the builders, the runner and the oracle of the four kinds live in tests/_sequence_plan.py, which the second sequence test
# (tests/test_gpu_sequence_all.py) and its CPU check share
from _sequence_plan import _ANCHOR, _QUANTUM_SHAPE, _data, _env_engine, _oracle, _penalties, _random_call, _run, _tensors

pytestmark = pytest.mark.gpu


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
