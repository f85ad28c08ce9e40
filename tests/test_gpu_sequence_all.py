"""GPU: one long-lived context through every entry point, in a seeded plan with directed adjacencies.

tests/test_gpu_sequence.py keeps one context alive through fused calls, VPP + rSGM, the occlusion heuristic and the post stage.
Every entry point added since put state of its own into the context: the resize tables and their key, three independent "which
set does the next pipelined call write" toggles, WS_DSI / WS_GUIDED_MAP / WS_PATHS that guided, fused and stage calls reserve
differently, the hand-off scratch the host entries stage through, the partial records of the metrics, the PNG offsets kept for
an asynchronous upload, the evaluation pointers in the graph key.  Each of them is held to its referee by a file of its own on
an engine that runs nothing else.  Here the plan of tests/_sequence_plan.py runs all of them on ONE engine per configuration,
with fixed adjacencies aimed at each item of state and a random tail around them, and every output of every call must equal the
same call on a fresh engine bit for bit.  The fresh-engine outputs are held to each feature's own referee once per seed.
tests/test_sequence_plan_cpu.py checks the plan itself without a GPU."""
import contextlib

import numpy as np
import pytest

import _sequence_plan as P

pytestmark = pytest.mark.gpu

_PREPARED = {}


def _prepared(seed):
    """(specs, order, marks, host data, reference outputs, reference route lists): each reference is the call on a fresh engine,
    closed before the next is made."""
    if seed not in _PREPARED:
        import torch
        probe = P._env_engine()
        quantum = probe.batch_quantum(*P._QUANTUM_SHAPE)
        probe.ctx.close()
        assert quantum >= 8, quantum
        specs, order, marks = P.plan(seed, quantum)
        datas = P.plan_data(specs)
        refs, routes = [], []
        for i, s in enumerate(specs):
            eng = P._env_engine()
            t, bufs = P.plan_tensors(eng, specs, datas, i, {})
            out = P.run(eng, s, datas[i], t, bufs)
            torch.cuda.synchronize()
            refs.append({k: v.cpu() for k, v in out.items()})
            routes.append((eng.last_routes(), eng.last_front_routes()))
            eng.ctx.close()
        _PREPARED[seed] = (specs, order, marks, datas, refs, routes)
    return _PREPARED[seed]


def _what(s):
    return {k: s[k] for k in ("kind", "role", "mode", "what", "B", "H", "W", "D", "gocc", "iscale", "oscale", "dtype", "shape") if k in s}


@pytest.mark.parametrize("seed", P.SEEDS)
def test_fresh_engine_references_match_the_referees(seed):
    """The references every configuration is held to: frames 0 and B - 1 of every call against the referee of the feature's own
    test (the CPU oracle, the metrics bound, the resize restatement, the float64 hand-off referee and its bfloat16 band, the
    pyramid and lookup referee, the pictures' restatement, torch's CPU sampler, the hand-built PNG files' samples)."""
    specs, order, marks, datas, refs, routes = _prepared(seed)
    assert {s["kind"] for s in specs} == set(P.ALL_KINDS), sorted({s["kind"] for s in specs})
    for i, (s, d, ref) in enumerate(zip(specs, datas, refs)):
        try:
            P.referee(s, d, {k: P.host_array(v) for k, v in ref.items()})
        except AssertionError as e:
            raise AssertionError(f"spec {i} {_what(s)}: {e}") from e
        if s["kind"] in P.HOT_KINDS + ("host",) and s.get("mode") != "metrics":
            assert ("scale_restore" in routes[i][0]) == (s["iscale"] != 1 and s["oscale"] != s["iscale"]), (i, routes[i][0])


def _bits(x):
    """A tensor as integers of its own width: NaN cells compare by their bits."""
    import torch
    view = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16}.get(x.dtype)
    return x.contiguous().view(view) if view is not None else x


@pytest.mark.parametrize("config", P.CONFIGS, ids=[c[0] for c in P.CONFIGS])
@pytest.mark.parametrize("seed", P.SEEDS)
def test_one_context_through_every_entry_point(seed, config):
    """One engine runs the whole plan (pipelined: with no synchronisation between calls and the inputs-ready event of every hot-path call, so that front stages overlap
    the call before; graph mode: on a side stream); every
    output of every call equals the fresh-engine reference, and so do the route lists a call leaves.  The paths are shown taken:
    the resize tables are built once per change of shape and reused in between, the aggregation layout changes within the
    default and pipelined sequences, the call across the lock-step round runs in parts, the workspace grows, and the graph
    replays fall where the key says they must -- behind calls that changed nothing the key holds, not on calls that differ from
    the anchor in metrics_out or in gt alone, not behind the call that grew the workspace."""
    import torch
    name, env, pipelined, graph = config
    specs, order, marks, datas, refs, ref_routes = _prepared(seed)
    eng = P._env_engine(**env)
    side = torch.cuda.Stream(device=eng.device) if graph else None
    layouts, replays, grew, builds, parts, routes, sets = set(), [], [], [], [], [], []
    got = []
    try:
        if pipelined:
            eng.set_pipeline(True)
        if graph:
            eng.set_graph_mode(True)
        ws = lambda: int(eng.lib.vppx_workspace_bytes(eng.ctx.handle))
        with torch.cuda.stream(side) if graph else contextlib.nullcontext():
            cache = {}
            tens = [P.plan_tensors(eng, specs, datas, i, cache) for i in range(len(specs))]
            torch.cuda.current_stream(eng.device).synchronize()
            # pipelined: every input of the plan exists behind this event, and the calls of the hot path say so, which is what lets
            # a front stage start next to the call before (else it waits for everything queued so far)
            ready = None
            if pipelined:
                ready = torch.cuda.Event()
                ready.record()
            for pos, i in enumerate(order):
                s = specs[i]
                r0, w0, b0 = eng.graph_replays(), ws(), eng.scale_table_builds()
                before = (eng.last_routes(), eng.last_front_routes())
                got.append(P.run(eng, s, datas[i], *tens[i], ready=ready))
                if not pipelined and not graph:
                    eng.synchronize()
                if s["kind"] in ("fused", "split") + P.HOT_KINDS:
                    layouts.add(eng.uses_vert())
                parts.append(eng.last_call_parts())
                replays.append(eng.graph_replays() - r0)
                grew.append(ws() > w0)
                builds.append(eng.scale_table_builds() - b0)
                routes.append((before, (eng.last_routes(), eng.last_front_routes())))
                sets.append(eng.last_front_sets())
            eng.synchronize()
        kinds = [specs[i]["kind"] for i in order]
        print(f"\n[{seed}-{name}] {len(order)} calls of {len(specs)} specs; kinds: {' '.join(kinds)}")
        print(f"[{seed}-{name}] graph replays per position: {replays}")
        print(f"[{seed}-{name}] table builds per position: {builds}; workspace grew at: {[p for p, g in enumerate(grew) if g]}")
        for pos, i in enumerate(order):
            assert got[pos].keys() == refs[i].keys(), (name, pos, i)
            for k, w in refs[i].items():
                g = got[pos][k].cpu()
                assert g.dtype == w.dtype and g.shape == w.shape, (name, pos, i, k)
                assert torch.equal(_bits(g), _bits(w)), (name, pos, i, k, _what(specs[i]), int((_bits(g) != _bits(w)).sum()))
        if name in ("default", "pipelined", "graph"):       # (sub-stream children keep lists of their own; VPPX_VERT=0 takes other routes)
            for pos, i in enumerate(order):
                before, after = routes[pos]
                for n in (0, 1):
                    if (specs[i]["kind"] in P.ROUTE_KINDS and specs[i].get("mode") != "metrics") or ref_routes[i][n]:
                        assert after[n] == ref_routes[i][n], (name, pos, i, n, _what(specs[i]), after[n], ref_routes[i][n])
                    else:       # a call that launches no such kernel neither clears nor extends the list
                        assert after[n] == before[n], (name, pos, i, n, _what(specs[i]), before[n], after[n])
        # the resize tables: built for A, reused by A, rebuilt for another shape and again for A; a hand-off call and a growing
        # call in between leave them where they are
        assert [builds[p] for p in marks["tables"]] == [1, 0, 1, 1, 0, 0, 0, 0], [builds[p] for p in marks["tables"]]
        keys = [k for k in _scaled_keys(specs, order) if k is not None]
        assert sum(builds) == sum(1 for a, b in zip([None] + keys, keys) if a != b), (builds, keys)
        # the two sets of scaled and of sampled maps: consecutive resizing calls, and consecutive sampling calls, of a pipelined
        # context alternate (the next front stage may write while this call's guided rows still read); every other context
        # writes set 0.  Values cannot show this at these sizes -- the reader is through in microseconds -- so the set is read out.
        resizing = [p for p, i in enumerate(order) if specs[i].get("iscale", 1) != 1]
        sampling = [p for p, i in enumerate(order) if specs[i].get("sample") is not None]
        assert len(resizing) >= 10 and len(sampling) >= 6
        for which, at in ((0, resizing), (1, sampling)):
            want = [k % 2 if pipelined else 0 for k in range(len(at))]
            assert [sets[p][which] for p in at] == want, (name, which, [sets[p][which] for p in at])
        if name in ("default", "pipelined"):
            assert len(layouts) >= 2, layouts
        if name == "default":
            assert parts[marks["crossing"][0]] > 1, parts
        role = [specs[i].get("role") for i in order]
        pg = role.index("grow")
        assert grew[pg], "the growing call did not grow the workspace"
        assert grew[marks["tables"][6]], "the growing call of the tables part did not grow the workspace"
        if graph:
            g0, g1 = marks["graph"][0], marks["graph"][-1]
            want = P.expected_replays(order, specs, grew, g0, g1)
            assert replays[g0:g1 + 1] == want, (replays[g0:g1 + 1], want, role[g0:g1 + 1])
            # and what that means at the adjacencies: a replay of the anchor right behind each call that left the key alone ...
            for r in ("other_metrics", "other_gt", "between"):
                for p in (p for p in marks["graph"] if role[p] == r):
                    assert replays[p] == 0 and role[p + 1] == "anchor" and replays[p + 1] == 1, (r, p, replays[g0:g1 + 1])
            # ... none right behind the call that grew the workspace, and the next one captured again and launched
            assert role[pg + 1:pg + 3] == ["anchor", "anchor"] and replays[pg:pg + 3] == [0, 0, 1], replays[pg:pg + 3]
            assert sum(replays) >= 3, replays
        else:
            assert not any(replays), replays
    finally:
        if graph:
            eng.set_graph_mode(False)
        torch.cuda.synchronize()
        eng.ctx.close()


def _scaled_keys(specs, order):
    """Per position, the (H, W, iscale, oscale) of a call that resizes, else None."""
    out = []
    for i in order:
        s = specs[i]
        out.append((s["H"], s["W"], s["iscale"], s["oscale"]) if s.get("iscale", 1) != 1 else None)
    return out
