"""The plan of tests/test_gpu_sequence_all.py, checked without a GPU: that it holds every kind of call and the seven adjacencies in
their order, that calls share arrays only where the plan says they are one call, that the data builders deliver what the plan
relies on, and that every referee the GPU test holds its references to runs on the plan's data (tests/_sequence_plan.py)."""
import numpy as np
import pytest

import _sequence_plan as P

QUANTUM = 13            # batch_quantum of the crossing shape is asked of the device; any value >= 8 gives a plan of the same shape
_PLANS = {}


def _plan(seed):
    if seed not in _PLANS:
        specs, order, marks = P.plan(seed, QUANTUM)
        _PLANS[seed] = (specs, order, marks, P.plan_data(specs))
    return _PLANS[seed]


def _calls(seed, name):
    specs, order, marks, _ = _plan(seed)
    return [specs[order[p]] for p in marks[name]]


@pytest.mark.parametrize("seed", P.SEEDS)
def test_plan_contains_every_kind_and_stays_small(seed):
    specs, order, marks, _ = _plan(seed)
    assert {s["kind"] for s in specs} == set(P.ALL_KINDS)
    assert order == P.plan(seed, QUANTUM)[1]                                       # seeded: the same plan again
    assert 60 <= len(order) <= 80
    crossing = _calls(seed, "crossing")[0]
    for s in specs:
        if s is crossing:
            continue
        assert s.get("B", 1) <= 16 and s.get("D", 0) <= 256, s
        assert s.get("H", s.get("Ho", 0)) <= 64 and s.get("W", s.get("Wo", 0)) <= 330, s
    assert crossing["B"] == 2 * QUANTUM + 1 and (crossing["H"], crossing["W"], crossing["D"]) == P._QUANTUM_SHAPE


@pytest.mark.parametrize("seed", P.SEEDS)
def test_the_seven_adjacencies_are_in_the_order_stated(seed):
    specs, order, marks, _ = _plan(seed)
    assert list(marks) == ["variations", "tables", "parities", "hazards", "dsi", "handoff", "png", "graph", "crossing"]
    flat = [p for m in marks.values() for p in m]
    assert flat == sorted(flat) and len(set(flat)) == len(flat)                   # the parts follow each other, each contiguous
    for m in marks.values():
        assert m == list(range(m[0], m[-1] + 1))
    # 1. A, A, another shape, A, hand-off, A, a growing call, A
    t = _calls(seed, "tables")
    A = t[0]
    assert [x is A for x in t] == [True, True, False, True, False, True, False, True]
    assert A["kind"] == t[2]["kind"] == "scaled" and A["iscale"] != 1 and t[2]["iscale"] != 1
    assert (A["H"], A["W"], A["iscale"], A["oscale"]) != (t[2]["H"], t[2]["W"], t[2]["iscale"], t[2]["oscale"])
    assert t[4]["kind"] == "handoff" and t[6]["kind"] == "fused" and t[6]["B"] * t[6]["H"] * t[6]["W"] * t[6]["D"] > 8 * A["B"] * A["H"] * A["W"] * A["D"]
    # 2. plain fused, scaled, sampled, plain fused: pipelined-eligible (the fused layout's batch), different data per call
    p = _calls(seed, "parities")
    assert [x["kind"] for x in p] == ["fused", "scaled", "sampled", "fused"] and all(x["B"] >= 8 for x in p)
    assert p[1]["iscale"] != 1 and p[2]["sample"] is not None and len({x["data"] for x in p}) == 4 and len({x["seed"] for x in p}) == 4
    assert p[2]["iscale"] == 2                                                      # the sampled call that also resizes
    # 2b. two scaled guided and two sampled guided calls of few frames back to back, the first again behind the second
    z = _calls(seed, "hazards")
    assert [x["kind"] for x in z] == ["fused"] + ["scaled"] * 3 + ["fused"] + ["sampled"] * 3 and z[4] is z[0]
    zs, zp = z[1:4], z[5:]
    assert zs[2] is zs[0] and zp[2] is zp[0] and all(x["B"] < 8 for x in zs + zp)
    assert all(x["guided"] for x in zs) and all(x["sample"]["guided"] for x in zp)
    assert zs[0]["data"] != zs[1]["data"] and zp[0]["data"] != zp[1]["data"] and zp[0]["sample"]["seed"] != zp[1]["sample"]["seed"]
    assert z[0]["B"] * z[0]["H"] * z[0]["W"] * z[0]["D"] > 50 * zs[0]["B"] * (zs[0]["H"] // 2) * (zs[0]["W"] // 2) * zs[0]["D"]    # busy
    # 3. guided at D = 256, the stage natives at D = 64, guided with a hint on every pixel, fused with byte volumes, guided without hints
    g = _calls(seed, "dsi")
    assert [x["kind"] for x in g] == ["guided", "stage", "guided", "fused", "guided"]
    assert g[0]["D"] == 256 and g[1]["D"] == 64 and g[2]["D"] == 64 and g[2]["p_hints"] == 1.0 and g[4]["p_hints"] == 0.0
    assert all(x["guided"] for x in (g[0], g[2], g[4]))
    assert 3 * (24 + max(g[3]["rsgm"]["p2min"], g[3]["rsgm"]["gamma"])) <= 255     # the sums of three paths fit a byte
    # 4. hand-off with hints, a host call with validhints, a smaller corr call with hints, a scaled host call, the hand-off again
    h = _calls(seed, "handoff")
    assert [x["kind"] for x in h] == ["handoff", "host", "corr", "host", "handoff"] and h[4] is h[0]
    assert h[0]["hints"] and h[1]["mode"] == "call" and h[1]["guided"] and h[2]["hints"] and h[3]["mode"] == "scaled"
    # 5. two PNG batches back to back, more partial records than ever before, then fewer
    q = _calls(seed, "png")
    assert [x["kind"] for x in q] == ["decode", "decode", "metrics", "eval"] and q[0]["what"] == q[1]["what"] == "png"
    before = [specs[i] for i in order[:marks["png"][2]]]
    records = lambda s: s["B"] * -(-(s.get("Ho", s.get("H", 0)) * s.get("Wo", s.get("W", 0))) // 4096)
    assert records(q[2]) > max((records(s) for s in before if s["kind"] == "metrics" or s.get("evaluate")), default=0) and records(q[3]) < records(q[2])
    # (and the evaluating call differs from the last call that uploaded a penalty table -- the scaled host call -- in alpha alone)
    last = [s for s in before if "rsgm" in s and s["kind"] in P.ROUTE_KINDS][-1]
    assert {k for k in ("p2min", "gamma", "alpha") if last["rsgm"][k] != q[3]["rsgm"][k]} == {"alpha"}
    # 6. the evaluating anchor with, in between: another metrics_out, another gt, a sampled call, a scaled call of its inner shape,
    #    the growing call
    role = [x.get("role") for x in _calls(seed, "graph")]
    assert role == ["anchor"] * 3 + ["other_metrics", "anchor", "other_gt", "anchor", "between", "anchor", "between", "anchor", "grow", "anchor", "anchor"]
    gr = _calls(seed, "graph")
    E = gr[0]
    assert all(x is E for x, r in zip(gr, role) if r == "anchor") and E["evaluate"]
    assert gr[3]["own_out"] == ("metrics",) and gr[3]["own_in"] == () and gr[5]["own_in"] == ("gt",) and gr[5]["own_out"] == ()
    assert gr[7]["sample"] is not None and gr[9]["iscale"] == 2 and (gr[9]["H"] // 2, gr[9]["W"] // 2) == (E["H"], E["W"])
    for x in gr[:11]:           # nothing but the growing call changes the penalty table: the graph's table stays the anchor's
        assert x["rsgm"] == E["rsgm"]
    big = lambda s: s.get("B", 1) * s.get("H", s.get("Ho", 1)) * s.get("W", s.get("Wo", 1)) * s.get("D", 1)
    assert big(gr[11]) > max(big(specs[i]) for i in order[:marks["graph"][11]])    # the largest call so far
    # 7. the crossing call evaluates
    assert _calls(seed, "crossing")[0]["evaluate"]


@pytest.mark.parametrize("seed", P.SEEDS)
def test_calls_share_arrays_only_where_the_plan_says_so(seed):
    specs, order, marks, datas = _plan(seed)
    owner = {}
    for i, (s, d) in enumerate(zip(specs, datas)):
        for k, v in d.items():
            if not isinstance(v, np.ndarray):
                continue
            if id(v) in owner:
                j = owner[id(v)]
                assert s.get("shares") == specs[j].get("role") and k not in s["own_in"], (i, j, k)
            else:
                owner[id(v)] = i
    # two specs are one call only when they are one object; data that merely look alike are distinct arrays
    E = next(s for s in specs if s.get("role") == "anchor")
    Eg = next(s for s in specs if s.get("role") == "other_gt")
    dE, dG = datas[specs.index(E)], datas[specs.index(Eg)]
    assert dG["left"] is dE["left"] and dG["gt"] is not dE["gt"] and not np.array_equal(dG["gt"], dE["gt"])


@pytest.mark.parametrize("seed", P.SEEDS)
def test_the_data_builders_deliver_what_the_plan_relies_on(seed):
    specs, order, marks, datas = _plan(seed)
    of = lambda s: datas[next(i for i, x in enumerate(specs) if x is s)]
    # the hint densities
    for s, d in zip(specs, datas):
        if s["kind"] in P.HOT_KINDS + ("host",) and "hints" in d:
            dens = float((d["hints"] > 0).mean())
            if s["p_hints"] == 0.0:
                assert dens == 0.0
            elif s["p_hints"] == 1.0:
                assert dens == 1.0
            else:
                assert abs(dens - s["p_hints"]) < 0.6 * s["p_hints"], (dens, s["p_hints"])
            if s["guided"]:
                assert np.array_equal(d["validhints"] > 0, d["hints"] > 0)
        if s.get("evaluate"):
            assert set(np.unique(d["validgt"])) == {-1.0, 0.0, 0.5, 1.0}
    # a RAFT row with v == 0, and the W4 = 12 / 16 shapes, in the hand-off calls of the plan
    hand = [s for s in specs if s["kind"] == "handoff"]
    assert any((of(s)["_cases"][1].v4 == 0).any() and (of(s)["_cases"][1].v4 != 0).any() for s in hand)
    assert {of(s)["_cases"][0].W4 for s in hand} >= {12, 16}
    assert {s["dtype"] for s in hand} == {"float32", "bfloat16"}
    # metrics on both sides of one block per frame, unaligned batches
    npx = [s["Ho"] * s["Wo"] for s in specs if s["kind"] == "metrics"] + [s["H"] * s["W"] for s in specs if s.get("evaluate")]
    assert min(npx) <= 4096 < max(npx)
    # the two PNG batches differ in file count and size
    a, b = (of(s) for s in _calls(seed, "png")[:2])
    assert len(a["_offs"]) != len(b["_offs"]) and a["_hw"] != b["_hw"] and a["blob"].size != b["blob"].size
    # a scaled shape whose restored map is not the frame's
    scaled = [s for s in specs if s.get("iscale", 1) != 1]
    assert any(P._hot_shape(s)[2] != s["H"] for s in scaled if s["oscale"] == 1)
    assert {(s["iscale"], s["oscale"]) for s in scaled} >= {(2, 1), (2, 2), (3, 2), (3, 1)}
    assert any(s["H"] % 2 for s in scaled)
    # the sampling seed near 2^32, both sources
    assert any(s["seed"] >= 2 ** 32 - 2 for s in specs if s["kind"] == "sample")
    assert any(s["sample"]["seed"] >= 2 ** 32 - 2 for s in specs if s.get("sample"))
    c = _calls(seed, "handoff")[2]
    assert (c["levels"], c["radius"]) == (4, 4)
    # the stage call's frames, D = 64 in the fixed part
    st = _calls(seed, "dsi")[1]
    assert of(st)["_gl"].shape == (st["Hn"], st["Wn"]) and st["Wn"] % 16 == 0 and st["Wn"] >= st["D"]


@pytest.mark.parametrize("seed", P.SEEDS)
def test_every_variation_of_a_kind_occurs_in_the_fixed_part(seed):
    """What the plan must contain of every kind, counted over the named parts alone: the two calls drawn at random add to it and
    are not relied on."""
    specs, order, marks, datas = _plan(seed)
    fixed = []
    for m in marks.values():
        for p in m:
            if not any(specs[order[p]] is x for x in fixed):
                fixed.append(specs[order[p]])
    of = lambda s: datas[next(i for i, x in enumerate(specs) if x is s)]
    kind = lambda k: [s for s in fixed if s["kind"] == k]
    hotlike = [s for s in fixed if s["kind"] in P.HOT_KINDS]
    # guided: D in {8, 64, 160, 256}, hints 0 %, 5 %, every pixel, B from 1 up
    g = kind("guided")
    assert {s["D"] for s in g} >= {8, 64, 160, 256} and {s["p_hints"] for s in g} >= {0.0, 0.05, 1.0} and len({s["B"] for s in g}) >= 3
    # scaled: the four pairs, odd H, with and without validhints, with the heuristic and with a mask
    sc = [s for s in hotlike if s["iscale"] != 1 and s["sample"] is None and not s["evaluate"]]
    assert {(s["iscale"], s["oscale"]) for s in sc} >= {(2, 2), (2, 1), (3, 2), (3, 1)} and any(s["H"] % 2 for s in sc)
    assert {s["guided"] for s in sc} == {False, True} and {s["gocc"] for s in sc} >= {"none", "heuristic", "mask"}
    assert any(P._hot_shape(s)[2] != s["H"] for s in sc if s["oscale"] == 1)
    # eval: oscale 1 and 2, the float mask
    ev = [s for s in hotlike if s["evaluate"] and s["sample"] is None]
    assert {s["oscale"] for s in ev} >= {1, 2} and all(set(np.unique(of(s)["validgt"])) == {-1.0, 0.0, 0.5, 1.0} for s in ev)
    # sampled: guided on and off, from src and from gt, with the maps returned, with iscale = 2, with gt=
    sm = [s for s in hotlike if s["sample"] is not None]
    assert {s["sample"]["guided"] for s in sm} == {False, True} and {s["sample"]["source"] for s in sm} == {"src", "gt"}
    assert any(s["sample"]["outs"] for s in sm) and any(s["iscale"] == 2 for s in sm) and any(s["evaluate"] for s in sm)
    # metrics alone: both sides of 4096 pixels, gt_scale 1, 2, 3, B = 3 at odd H * W
    me = kind("metrics")
    assert min(s["Ho"] * s["Wo"] for s in me) <= 4096 < max(s["Ho"] * s["Wo"] for s in me) and {s["gt_scale"] for s in me} >= {1, 2, 3}
    assert any(s["B"] == 3 and (s["Ho"] * s["Wo"]) % 2 for s in me)
    # pictures: dilation 0, 1, 7; a frame smaller and one larger than a tile (16 x 16)
    vz = kind("viz")
    assert {s["dilation"] for s in vz} >= {0, 1, 7} and min(s["H"] for s in vz) < 16 and max(s["W"] for s in vz) > 256
    # sample_hints: p 0.05 and 1.0, a seed near 2^32
    sp = kind("sample")
    assert {s["p"] for s in sp} >= {0.05, 1.0} and any(s["seed"] >= 2 ** 32 - 2 for s in sp)
    # hand-off: both dtypes, with and without hints, W4 12 and 16, a RAFT row with v == 0
    ho = kind("handoff")
    assert {s["dtype"] for s in ho} == {"float32", "bfloat16"} and {s["hints"] for s in ho} == {False, True}
    assert {of(s)["_cases"][0].W4 for s in ho} >= {12, 16} and any((of(s)["_cases"][1].v4 == 0).any() for s in ho)
    # pyramid and lookup: levels 1 and 4, radius 0 and 4, both dtypes, with hints
    co = kind("corr")
    assert {s["levels"] for s in co} >= {1, 4} and {s["radius"] for s in co} >= {0, 4} and {s["dtype"] for s in co} == {"float32", "bfloat16"}
    assert any(s["hints"] for s in co)
    # decoders: two PNG batches, PFM, KITTI
    de = kind("decode")
    assert {s["what"] for s in de} == {"png", "pfm", "kitti"} and sum(s["what"] == "png" for s in de) >= 2
    # stage entries and natives: D 64 and 256
    assert {s["D"] for s in kind("stage")} >= {64, 256}
    # the _host twins: the call (with validhints), the scaled call (with the heuristic), the metrics
    hs = kind("host")
    assert {s["mode"] for s in hs} == {"call", "scaled", "metrics"}
    assert any(s["guided"] for s in hs if s["mode"] == "call") and any(s["gocc"] == "heuristic" for s in hs)
    # and the four kinds of the first plan: a split, an occlusion and a post call come in front of the parts
    assert {specs[i]["kind"] for i in order[:marks["variations"][0]]} == {"split", "occ", "post"}
    assert kind("fused")


@pytest.mark.parametrize("seed", P.SEEDS)
def test_every_referee_runs_on_the_plans_data(seed):
    """A dry run: the oracle, the metrics, the resize restatement, the hand-off referee and its band, the pyramid and lookup, the
    pictures, the CPU sampler and the PNG samples are all computed for frames 0 and B - 1 of every call; nothing is compared."""
    specs, order, marks, datas = _plan(seed)
    for s, d in zip(specs, datas):
        P.referee(s, d, None)


def test_expected_replays_follow_the_key_rule():
    """The model the GPU test holds the replay counts to, on the graph block alone with a workspace that grows at the growing call
    and at the anchor's first occurrence."""
    specs, order, marks, _ = _plan(0)
    g = marks["graph"]
    grew = [False] * len(order)
    grew[g[0]] = grew[g[11]] = True
    assert P.expected_replays(order, specs, grew, g[0], g[-1]) == [0, 1, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1]
    grew[g[7]] = True           # were the sampled call to grow the workspace, the anchor behind it would run eagerly and be captured again
    assert P.expected_replays(order, specs, grew, g[0], g[-1]) == [0, 1, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1]
