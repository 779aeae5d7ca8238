"""CPU: the launch schedule of ops.gemm().  ops.plan_gemm() is held to the launches the commit named in tests/golden/gemm_launch_plans.json made
of every catalogue case (tools/record_gemm_launch_plans.py recorded them there by running that commit's gemm() on stand-in operands), and the executor
is driven with the same stand-ins: what it hands to _gemm_one, in which order, around which fork / join, and what happens to the split-K scratch."""
import importlib.util
import itertools
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("TAIL_SPLIT", "TAIL_SPLIT_K", "TAIL_SIDE_STREAM", "K64_CFG14", "HALF_HEIGHT_SHORT_K", "HALF_HEIGHT_SHORT_K_ALWAYS", "SHORT_K_WIDE_HALF_N",
         "SHORT_K_WIDE_HALF_BYTES", "SHORT_K_WIDE_HALF_STASH", "CHAINS", "QUAD", "QUADV", "RING5", "PERSIST_STORE_ONLY", "KBLOCK_W", "TILE_GROUP")
SETTINGS = ({"TAIL_SPLIT": False}, {"TAIL_SPLIT_K": False}, {"TAIL_SIDE_STREAM": False}, {"K64_CFG14": False}, {"HALF_HEIGHT_SHORT_K": False},
            {"HALF_HEIGHT_SHORT_K_ALWAYS": True}, {"SHORT_K_WIDE_HALF_N": 0}, {"SHORT_K_WIDE_HALF_BYTES": 1536}, {"SHORT_K_WIDE_HALF_STASH": False}, {"CHAINS": 3},
            {"QUAD": True}, {"QUADV": 27}, {"QUADV": 29}, {"RING5": True}, {"PERSIST_STORE_ONLY": True}, {"KBLOCK_W": False}, {"TILE_GROUP": {"768": 4}})


@pytest.fixture(scope="module")
def plans():
    """the fixture, spelled out: cases = [M, N, K, esz, ncu, tile_cfg, epilogue name], default[i] = launches of case i, varied = the cases the knob
    settings were recorded on, knobs[j]["diffs"] = {case: launches} where setting j changed them"""
    with open(os.path.join(ROOT, "tests", "golden", "gemm_launch_plans.json")) as f:
        doc = json.load(f)
    doc["cases"], doc["varied"] = [], []
    for b in doc["blocks"]:
        new = [[M, N, K, esz, ncu, cfg, epi] for ncu, esz, M, (N, K), cfg, epi in itertools.product(*(b[k] for k in ("ncu", "esz", "M", "NK", "tile_cfg", "epi")))]
        doc["varied"] += range(len(doc["cases"]), len(doc["cases"]) + len(new)) if b["knobs"] else []
        doc["cases"] += new
    doc["default"] = [doc["plans"][p] for p in doc["default"]]
    for k in doc["knobs"]:
        assert len(k["cases"]) == len(k["plans"]) and set(k["cases"]) <= set(doc["varied"])
        k["diffs"] = {i: doc["plans"][p] for i, p in zip(k["cases"], k["plans"])}
    return doc


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_gemm_launch_plans", os.path.join(ROOT, "tools", "record_gemm_launch_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kinds(case, launches):
    """which kinds of plan the recorded launches of one case show (kernel cfg = what the GEMM_PROFILE tap named)"""
    out = {"cfg %d" % l[6] for l in launches if l[6] in (16, 23)}
    if case[5]:
        return out
    if len(launches) == 1:
        out.add("whole launch on cfg 14" if launches[0][2] & 255 == 14 else "single")
    else:
        out.add("tail on the side stream" if any(l[4] for l in launches) else "tail behind the main launch")
        if any(l[5] for l in launches):
            out.add("tail split over K")
    return out


def test_fixture_is_not_vacuous(plans):
    """The catalogue holds what the issue asks of it: the step's shapes, each kind of plan under default knobs, and for every knob at least one case whose
    launches the knob changes."""
    cases, default = plans["cases"], plans["default"]
    assert len(plans["commit"]) >= 40 and len(cases) == len(default)
    plain = [c for c in cases if c[5] == 0 and c[6] == "out_t"]
    for i, want in enumerate(((50432, 43520, 65536, 32896, 25216, 12608, 4096, 2048, 788, 256), (64, 768, 1024, 2304, 3072, 4096), (64, 768, 1024, 3072, 4096), (2, 4), (256, 304))):
        assert set(want) <= {c[i] for c in plain}
    assert len(plain) >= 10 * 6 * 5 * 2 * 2
    assert {13, 3 | 4 << 16 | 1 << 22} <= {c[5] for c in cases}
    assert {"out_t", "bias_gelu_aux", "resid_out32_rowsum", "resid3_out_lo", "drop_acc", "drop_a", "out_group", "resid_mod", "ext_a2", "rmw_out_t", "rmw_out32"} <= {c[6] for c in cases}
    seen = set()
    for c, l in zip(cases, default):
        seen |= kinds(c, l)
    assert seen >= {"single", "tail behind the main launch", "tail on the side stream", "tail split over K", "whole launch on cfg 14", "cfg 23", "cfg 16"}
    assert [k["set"] for k in plans["knobs"]] == list(SETTINGS)
    for k in plans["knobs"]:
        assert k["diffs"] and all(v != default[i] for i, v in k["diffs"].items()), k["set"]


def test_plan_gemm_matches_the_recorded_launches(plans):
    """ops.plan_gemm(), given plain values only, names exactly the launches the recorded commit's gemm() made: rows, tile_cfg word, K-blocked weight, side
    stream, split-K scratch — and the tile config the GEMM_PROFILE tap reports for it — for every case under default knobs and under every knob setting."""
    from uia_hip import ops
    cases, epi = plans["cases"], plans["epilogues"]
    saved = {k: getattr(ops, k) for k in KNOBS}

    def check(which, expected):
        for i in which:
            M, N, K, esz, ncu, tile_cfg, name = cases[i]
            got = ops.plan_gemm(M, N, K, esz, ncu, tile_cfg, **epi[name]["facts"])
            want, mask = expected(i), epi[name]["mask"]
            assert len(got) == len(want), (cases[i], got, want)
            for L, (lo, hi, word, w_kb, side, scratch, kernel) in zip(got, want):
                # the tap refines the launcher's own choice with the epilogue mask the descriptor turned out to have (N = 64: stream kernel or not)
                reported = L.base if (L.tile_cfg & 255 or L.base == 23) else ops.auto_tile_cfg(hi - lo, N, K, esz, mask)
                assert (L.lo, L.hi, L.tile_cfg, int(L.w_kblocked), int(L.side), L.scratch, reported) == (lo, hi, word, w_kb, side, scratch, kernel), (cases[i], got, want)

    try:
        check(range(len(cases)), lambda i: plans["default"][i])
        for k in plans["knobs"]:
            for name, v in k["set"].items():
                setattr(ops, name, {int(n): g for n, g in v.items()} if isinstance(v, dict) else v)
            check(plans["varied"], lambda i: k["diffs"].get(i, plans["default"][i]))
            for name in k["set"]:
                setattr(ops, name, saved[name])
    finally:
        for name, v in saved.items():
            setattr(ops, name, v)


def test_plan_gemm_of_a_direct_launch_does_not_split(plans):
    """whole=True is what _gemm_one asks for when it is called with a tile_cfg of its own: one launch of all rows, same resolution of the word."""
    from uia_hip import ops
    L, = ops.plan_gemm(32896, 1024, 4096, 2, 0, 0, whole=True, packed=True, out_t=True)
    assert (L.lo, L.hi, L.tile_cfg, L.base, L.w_kblocked, L.side, L.scratch) == (0, 32896, 8, 8, True, False, 0)
    L, = ops.plan_gemm(128, 1024, 4096, 2, 0, 13 | 8 << 16 | 1 << 22, whole=True, packed=True, out_t=True)
    assert (L.tile_cfg, L.base, L.w_kblocked) == (13 | 8 << 16 | 1 << 22, 13, True)
    L, = ops.plan_gemm(50432, 768, 64, 2, 0, 0, whole=True, packed=True, out_t=True, resid_t=True)
    assert (L.tile_cfg, L.base, L.w_kblocked) == (0, 23, False)


@pytest.mark.parametrize("case", [(4096, 768, 768, "bias_gelu_aux"), (50432, 3072, 3072, "resid_out32_rowsum"), (32896, 4096, 1024, "resid3_out_lo"),
                                  (32896, 1024, 4096, "resid3_out_lo"), (50432, 768, 768, "kblocked_lnfold"), (50432, 768, 64, "rmw_out_t"), (50432, 64, 768, "out_t"),
                                  (32896, 1024, 1024 + 64, "ext_a2_groups")], ids=lambda c: "%dx%dx%d-%s" % c)
def test_gemm_executor_walks_the_plan(recorder, case):
    """ops.gemm() on stand-in operands: every launch of the plan reaches _gemm_one once, in the plan's order, with every row-indexed operand cut to the
    launch's rows (and nothing cut when the plan is one launch); launches marked `side` sit inside one fork that is opened before anything else is
    enqueued and joined after the last launch; the split-K scratch is obtained once, inside the fork when the tail is on the side stream."""
    from uia_hip import ops
    M, N, K, name = case
    a, w, kw = recorder.operands(M, N, K, 2, name)
    ops._NCU[0] = 256
    plan = ops.plan_gemm(M, N, K, 2, 256, 0, **recorder.EPILOGUES[name]["facts"])
    orig, seen = ops._gemm_one, []

    def rows_of(t):
        return None if t is None else (t.rows if ops.is_kb(t) else t.shape[-2])

    def spy(a_, w_, **k):
        assert w_ is w
        seen.append(k)
        rec.events.append(("one", k["launch"]))
        rows = k["launch"].hi - k["launch"].lo
        cut = [a_, (k.get("a2") or (None,))[0]] + [k.get(n) for n in ("aux_in", "aux_out", "resid", "resid_t", "out_t", "out32", "rowsum", "out_lo")]
        cut += [k[n][0] for n in ("resid_ln", "lnfold") if k.get(n) is not None] + list(k.get("resid3") or ())
        assert {rows_of(t) for t in cut if t is not None} == {rows}, (k["launch"], [rows_of(t) for t in cut])
        return orig(a_, w_, **k)

    try:
        ops._gemm_one = spy
        with recorder.Recorder() as rec:
            ops.gemm(a, w, **kw)
    finally:
        ops._gemm_one = orig
        ops._NCU.pop(0, None)
    assert [k["launch"] for k in seen] == plan
    if len(plan) == 1:
        assert seen[0]["out_t"] is kw["out_t"] and not any(e[0] in ("fork", "join", "scratch") for e in rec.events)
    launched = [e[1] for e in rec.events if e[0] == "launch"]
    assert [(c["M"], c["tile_cfg"], c["w_kblocked"], c["side"], c["scratch"]) for c in launched] == [(L.hi - L.lo, L.tile_cfg, int(L.w_kblocked), L.side, L.scratch) for L in plan]
    # row ranges, from the addresses: `a` and the outputs start at row lo
    for c, L in zip(launched, plan):
        out = kw["out_t"] if "out_t" in kw else kw["out32"]
        step = 64 if ops.is_kb(a) else a.stride(0) * 2
        assert c["A"] - a.data_ptr() == L.lo * step
        if ops.is_kb(out):
            assert c["outT"] - out.data_ptr() == L.lo * 64
        else:
            assert (c["outT"] or c["out32"]) - out.data_ptr() == L.lo * out.stride(0) * out.element_size()
    order = [e[0] if e[0] != "one" else ("side" if e[1].side else "main") for e in rec.events if e[0] in ("fork", "side done", "join", "one", "scratch")]
    n_side = sum(L.side for L in plan)
    if n_side:
        want = ["fork"] + (["scratch"] if plan[0].scratch else []) + ["side"] * n_side + ["side done"] + ["main"] * (len(plan) - n_side) + ["join"]
    else:
        want = ["main"] * (len(plan) - sum(1 for L in plan if L.scratch)) + (["scratch"] if any(L.scratch for L in plan) else []) + ["main"] * sum(1 for L in plan if L.scratch)
    assert order == want


def test_gemm_executor_drops_the_scratch_when_a_split_k_phase_fails(recorder):
    """An exception out of the phase-2 (or phase-1) launch of a split-K tail drops the shared scratch before it is re-raised, the fork is left, and nothing
    else is enqueued; an exception out of a launch that uses no scratch drops nothing."""
    from uia_hip import ops
    a, w, kw = recorder.operands(32896, 1024, 4096, 2, "out_t")
    plan = ops.plan_gemm(32896, 1024, 4096, 2, 256, 0, **recorder.EPILOGUES["out_t"]["facts"])
    assert [(L.side, bool(L.scratch), L.tile_cfg >> 22) for L in plan] == [(True, True, 1), (True, True, 2), (False, False, 0)]
    for fail_at, dropped in ((1, True), (2, True), (3, False)):
        ops._NCU[0] = 256
        try:
            with recorder.Recorder(fail_at=fail_at) as rec:
                with pytest.raises(ops.UiaError, match="launch refused"):
                    ops.gemm(a, w, **kw)
        finally:
            ops._NCU.pop(0, None)
        names = [e[0] for e in rec.events]
        assert names.count("launch") == fail_at - 1 and ("drop scratch" in names) == dropped and "join" not in names
        assert names.index("side done") > (names.index("drop scratch") if fail_at < 3 else names.index("scratch"))
