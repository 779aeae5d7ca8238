"""Record which uia_gemm launches ops.gemm() turns a problem into, on the host, and write tests/golden/gemm_launch_plans.json.

No GPU: gemm() runs unmodified on stand-in operands (shape / stride / pointer arithmetic only) while the stream, the side-stream fork, the
split-K scratch, the LayerNorm guard word and the C library are replaced by recorders.  Run it on the commit whose behaviour is to be pinned
(the fixture names that commit); tests/test_gemm_plan_host.py then holds ops.plan_gemm() to the recorded launches, and uses the same stand-ins
to drive the executor.

    python tools/record_gemm_launch_plans.py            # rewrite the fixture from the checked-out commit
    python tools/record_gemm_launch_plans.py --check    # record again and compare with the committed fixture

Fixture layout: `blocks` spell the catalogue — the cases of a block are the product, in this order, of its ncu, esz, M, NK = [N, K] pairs, tile_cfg and
epi (epilogue name) lists, and the catalogue is the blocks' cases one after the other; `plans` is the table of distinct launch lists, one
[lo, hi, tile_cfg word, w_kblocked, side stream, split-K scratch floats, kernel cfg] per uia_gemm call in call order (kernel cfg is what the
GEMM_PROFILE tap reports; the epilogue mask it reports is a property of the epilogue class: `epilogues[name]["mask"]`); `default[i]` = index in `plans` of what case i became under default knobs; `knobs` = one record per knob setting
over the cases of the blocks marked "knobs": `cases` / `plans` name the cases whose launches differ from the default ones and what they became —
every other such case was recorded equal to its default.
"""
import argparse
import itertools
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextgen-uia_amd"))
from uia_hip import ops  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_launch_plans.json")
BF16, F32 = torch.bfloat16, torch.float32
_ESZ = {torch.bfloat16: 2, torch.float32: 4, torch.int8: 1, torch.int32: 4, torch.int64: 8}


class Dev:
    type, index = "cuda", 0


class T:
    """Stand-in for a device tensor: shape, strides and a made-up address; slicing moves the address like a view does."""
    _next = [1]
    is_cuda, device = True, Dev()

    def __init__(self, shape, dtype, strides=None, ptr=None):
        self.shape, self.dtype = tuple(shape), dtype
        if strides is None:
            strides, n = [], 1
            for s in reversed(self.shape):
                strides.insert(0, n)
                n *= s
        self._strides = tuple(strides)
        if ptr is None:
            ptr = T._next[0] << 40
            T._next[0] += 1
        self._ptr = ptr

    def dim(self):
        return len(self.shape)

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def element_size(self):
        return _ESZ[self.dtype]

    def data_ptr(self):
        return self._ptr

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def is_contiguous(self):
        return self._strides == T(self.shape, self.dtype, ptr=0)._strides

    def __getitem__(self, idx):
        idx = idx if isinstance(idx, tuple) else (idx,)
        if Ellipsis in idx:
            k = idx.index(Ellipsis)
            idx = idx[:k] + (slice(None),) * (self.dim() - len(idx) + 1) + idx[k + 1:]
        shape, ptr = list(self.shape), self._ptr
        for d, s in enumerate(idx):
            lo, hi, step = s.indices(shape[d])
            assert step == 1
            shape[d], ptr = max(hi - lo, 0), ptr + lo * self._strides[d] * self.element_size()
        return T(shape, self.dtype, self._strides, ptr)


class Packed(ops.PackedW):
    """a PackedW over stand-ins (no ready events)"""
    __slots__ = ()

    def __init__(self, row, kb):
        self._row, self._kb, self.ready, self.kb_ready = row, kb, None, None


class Ext(ops.ExtW):
    __slots__ = ()

    def __init__(self, kb, N, K, K2):
        self._kb, self.N, self.K, self.K2, self.ready = kb, N, K, K2, None


def kblocked(M, K, dtype):
    g = 64 // _ESZ[dtype]
    return ops.KBlocked(T((K // g, M, g), dtype))


# Epilogue classes: `facts` is what the schedule reads (the keywords of ops.plan_gemm), `also` names operands that only travel through the slicing.
EPILOGUES = {
    "out_t": dict(facts=dict(packed=True, out_t=True)),
    "out_t_plain_w": dict(facts=dict(out_t=True)),
    "bias_gelu_aux": dict(facts=dict(packed=True, out_t=True, act=True, aux_out=True), also=["bias"]),
    "resid_out32_rowsum": dict(facts=dict(packed=True, resid=True, out32=True, out_t=True, rowsum=True), also=["bias"]),
    "resid_out32_alpha": dict(facts=dict(packed=True, resid=True, out32=True, alpha=0.5)),
    "resid3_out_lo": dict(facts=dict(packed=True, out_t=True, rowsum=True, ln=True), also=["bias", "resid3", "resid_ln", "out_lo"], bf16_only=True),
    "kblocked_lnfold": dict(facts=dict(packed=True, out_t=True, ln=True, a_kb=True, out_t_kb=True), also=["bias", "lnfold"], kb=True),
    "dgelu": dict(facts=dict(packed=True, out_t=True, act=True), also=["aux_in", "dact"]),
    "drop_acc": dict(facts=dict(packed=True, out_t=True, resid_t=True, drop="acc")),
    "drop_a": dict(facts=dict(packed=True, out_t=True, drop="a"), also=["a_drop_out"]),
    "out_group": dict(facts=dict(packed=True, out32=True, out_group=196)),
    "resid_mod": dict(facts=dict(packed=True, out32=True, resid=True, resid_mod=197), also=["bias"]),
    "ext_a2": dict(facts=dict(ext=True, out_t=True), also=["bias"], bf16_only=True),
    "ext_a2_groups": dict(facts=dict(ext=True, out_t=True, resid=True, out32=True), also=["a2_groups"], bf16_only=True),
    "rmw_out_t": dict(facts=dict(packed=True, out_t=True, resid_t=True)),
    "rmw_out32": dict(facts=dict(packed=True, out32=True, resid=True)),
    "rmw_out32_drop": dict(facts=dict(packed=True, out32=True, drop="acc")),
}
EXT_K2 = 64

KNOB_SETTINGS = [dict(TAIL_SPLIT=False), dict(TAIL_SPLIT_K=False), dict(TAIL_SIDE_STREAM=False), dict(K64_CFG14=False), dict(HALF_HEIGHT_SHORT_K=False),
                 dict(HALF_HEIGHT_SHORT_K_ALWAYS=True), dict(SHORT_K_WIDE_HALF_N=0), dict(SHORT_K_WIDE_HALF_BYTES=1536), dict(SHORT_K_WIDE_HALF_STASH=False),
                 dict(CHAINS=3), dict(QUAD=True), dict(QUADV=27), dict(QUADV=29), dict(RING5=True), dict(PERSIST_STORE_ONLY=True), dict(KBLOCK_W=False),
                 dict(TILE_GROUP={768: 4})]


def blocks():
    Ms, Ns, Ks = (50432, 43520, 65536, 32896, 25216, 12608, 4096, 2048, 788, 256), (64, 768, 1024, 2304, 3072, 4096), (64, 768, 1024, 3072, 4096)
    cross = dict(M=list(Ms), NK=[[N, K] for N in Ns for K in Ks], tile_cfg=[0], epi=["out_t"])
    out = [dict(ncu=[256], esz=[2], knobs=True, **cross), dict(ncu=[256], esz=[4], knobs=False, **cross), dict(ncu=[304], esz=[2, 4], knobs=False, **cross)]
    NK = [[768, 768], [3072, 768], [768, 3072], [1024, 4096], [4096, 1024], [1024, 1024], [2304, 768], [64, 768], [768, 64], [1024, 64]]
    for name, e in EPILOGUES.items():
        if name != "out_t":
            nk = [[N, K + EXT_K2 if e["facts"].get("ext") else K] for N, K in NK if not (e.get("kb") and (K <= 64 or N <= 64))]
            out.append(dict(ncu=[256], knobs=True, esz=[2] if e.get("bf16_only") else [2, 4], M=[50432, 65536, 32896, 4096, 256], NK=nk, tile_cfg=[0], epi=[name]))
    given = [13, 8, 14, 3, 3 | 4 << 16 | 1 << 22, 13 | 6 << 16 | 2 << 22]
    out.append(dict(ncu=[256], knobs=True, esz=[2], M=[50432, 32896, 788], NK=[[768, 768], [1024, 4096], [768, 64]], tile_cfg=given, epi=["out_t", "resid_out32_rowsum"]))
    out.append(dict(ncu=[256], knobs=True, esz=[2], M=[32896], NK=[[1024, 4096 + EXT_K2]], tile_cfg=given, epi=["ext_a2"]))
    return out


def cases_of(block):
    return [[M, N, K, esz, ncu, cfg, epi] for ncu, esz, M, (N, K), cfg, epi in itertools.product(*(block[k] for k in ("ncu", "esz", "M", "NK", "tile_cfg", "epi")))]


def operands(M, N, K, esz, name):
    """(a, w, keywords) for ops.gemm(): stand-ins that present the epilogue class `name` on an [M, K] x [N, K] problem."""
    e = EPILOGUES[name]
    f, also = e["facts"], e.get("also", ())
    dt = BF16 if esz == 2 else F32
    g = 64 // esz
    kw = {}
    if f.get("ext"):
        a, w = T((M, K - EXT_K2), dt), Ext(T((K // g, N, g), dt), N, K, EXT_K2)
        G = 3 if N % 192 == 0 else 1
        kw["a2"] = (T((G, M, EXT_K2), dt), N // G) if "a2_groups" in also else (T((M, EXT_K2), dt), N)
    else:
        a = kblocked(M, K, dt) if f.get("a_kb") else T((M, K), dt)
        w = Packed(T((N, K), dt), T((K // g, N, g), dt)) if f.get("packed") else T((N, K), dt)
    rows = M // f["out_group"] * (f["out_group"] + 1) if f.get("out_group") else M
    if f.get("out_t"):
        kw["out_t"] = kblocked(M, N, dt) if f.get("out_t_kb") else T((rows, N), dt)
    if f.get("out32"):
        kw["out32"] = T((rows, N), F32)
    if f.get("resid"):
        kw["resid"] = T((f.get("resid_mod", 0) + 1 or M, N), F32) if f.get("resid_mod") else T((M, N), F32)
    if f.get("resid_t"):
        kw["resid_t"] = T((M, N), dt)
    if f.get("aux_out"):
        kw["aux_out"] = T((M, N), dt)
    if f.get("act"):
        kw["dact" if "dact" in also else "act"] = "gelu"
    if f.get("rowsum"):
        kw["rowsum"] = T((M, 2), torch.int64)
    if f.get("drop"):
        kw["drop"] = (f["drop"], 0.1, 7) + ((T((M, K), dt),) if "a_drop_out" in also else ())
    for k in ("out_group", "resid_mod", "alpha"):
        if k in f:
            kw[k] = f[k]
    if f.get("resid_mod"):
        kw["resid_row_off"] = 1
    if "bias" in also:
        kw["bias"] = T((N,), F32)
    if "aux_in" in also:
        kw["aux_in"] = T((M, N), dt)
    if "resid3" in also:
        kw["resid3"] = (T((M, N), BF16), T((M, N), torch.int8))
    if "out_lo" in also:
        kw["out_lo"] = T((M, N), torch.int8)
    if "resid_ln" in also:
        kw["resid_ln"] = (T((M, 2), torch.int64), T((N,), F32), T((N,), F32), N, 1e-5)
    if "lnfold" in also:
        kw["lnfold"] = (T((M, 2), torch.int64), T((N,), F32), K, 1e-5)
    return a, w, kw


class Recorder:
    """Replaces the device-facing pieces of uia_hip.ops; `events` is the ordered log of what gemm() did."""

    def __init__(self, fail_at=None):
        self.events, self.forked, self.fail_at, self.launches = [], False, fail_at, 0
        rec = self

        class Fork:
            def __init__(self, device):
                pass

            def __enter__(self):
                rec.forked = True
                rec.events.append(("fork",))
                return self

            def __exit__(self, *exc):
                rec.forked = False
                rec.events.append(("side done",))
                return False

            def join(self):
                rec.events.append(("join",))

        class Lib:
            @staticmethod
            def uia_gemm(stream, code, dref, tile_cfg):
                d = dref._obj
                rec.launches += 1
                if rec.fail_at == rec.launches:
                    raise ops.UiaError("recorder: launch refused")
                rec.events.append(("launch", dict(A=d.A, M=d.M, N=d.N, K=d.K, lda=d.lda, a_kb_rows=d.a_kb_rows, tile_cfg=tile_cfg, w_kblocked=d.w_kblocked,
                                                  side=rec.forked, scratch=rec.scratch if d.splitk_ws else 0, outT=d.outT, out32=d.out32)))
                return 0

        class Event:
            def __init__(self, **kw):
                pass

            def record(self, *a):
                pass

        self.scratch = 0
        self.patch = dict(_TailFork=Fork, lib=lambda: Lib, _stream=lambda: 0, ln_flag=lambda device: T((1,), torch.int32),
                          splitk_workspace=self._scratch, drop_splitk_workspace=lambda device: self.events.append(("drop scratch",)))
        self.event_cls = Event

    def _scratch(self, floats, device):
        self.scratch = floats
        self.events.append(("scratch", floats, self.forked))
        return T((floats,), F32)

    def __enter__(self):
        self.saved = {k: getattr(ops, k) for k in self.patch}
        self.saved_event, torch.cuda.Event = torch.cuda.Event, self.event_cls
        for k, v in self.patch.items():
            setattr(ops, k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(ops, k, v)
        torch.cuda.Event = self.saved_event
        return False


def record_case(case):
    """The launches ops.gemm() makes of one catalogue case under the knobs that are set now."""
    M, N, K, esz, ncu, tile_cfg, name = case
    a, w, kw = operands(M, N, K, esz, name)
    ops._NCU[0] = ncu
    saved, ops.GEMM_PROFILE = ops.GEMM_PROFILE, []
    try:
        with Recorder() as rec:
            ops.gemm(a, w, tile_cfg=tile_cfg, **kw)
        prof = ops.GEMM_PROFILE
    finally:
        ops.GEMM_PROFILE = saved
        ops._NCU.pop(0, None)
    calls = [e[1] for e in rec.events if e[0] == "launch"]
    assert len(calls) == len(prof)
    a_ptr = a.data_ptr()
    out = []
    for c, p in zip(calls, prof):
        lo = (c["A"] - a_ptr) // (64 if ops.is_kb(a) else c["lda"] * esz)
        assert (c["N"], c["K"]) == (N, K) and lo * (64 if ops.is_kb(a) else c["lda"] * esz) == c["A"] - a_ptr
        assert EPILOGUES[name].setdefault("mask", p[8]) == p[8]
        out.append([lo, lo + c["M"], c["tile_cfg"], c["w_kblocked"], int(c["side"]), c["scratch"], p[6]])
    return out


def record_all():
    bl = blocks()
    cases, varied = [], []
    for b in bl:
        new = cases_of(b)
        varied += range(len(cases), len(cases) + len(new)) if b["knobs"] else []
        cases += new
    table = {}
    index = lambda launches: table.setdefault(json.dumps(launches), len(table))
    default = [index(record_case(c)) for c in cases]
    knobs = []
    for setting in KNOB_SETTINGS:
        saved = {k: getattr(ops, k) for k in setting}
        try:
            for k, v in setting.items():
                setattr(ops, k, v)
            got = [(i, index(record_case(cases[i]))) for i in varied]
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
        diff = [(i, p) for i, p in got if p != default[i]]
        knobs.append(dict(set={k: ({str(n): g for n, g in v.items()} if isinstance(v, dict) else v) for k, v in setting.items()},
                          cases=[i for i, p in diff], plans=[p for i, p in diff]))
    return dict(epilogues={k: dict(facts=v["facts"], mask=v["mask"]) for k, v in EPILOGUES.items()}, blocks=bl, plans=[json.loads(k) for k in table], default=default, knobs=knobs)


def dumps(doc):
    """compact, in lines of moderate length: the file stays small and diffable"""
    js = lambda x: json.dumps(x, separators=(",", ":"))

    def wrapped(xs, n):
        return "[\n" + ",\n".join(",".join(js(x) for x in xs[i:i + n]) for i in range(0, len(xs), n)) + "\n]"
    knobs = ",\n".join('{"set":%s,"cases":%s,\n"plans":%s}' % (js(k["set"]), wrapped(k["cases"], 40), wrapped(k["plans"], 50)) for k in doc["knobs"])
    return ('{"what":%s,\n"commit":%s,\n"epilogues":%s,\n"blocks":%s,\n"plans":%s,\n"default":%s,\n"knobs":[\n%s\n]}\n'
            % (js(doc["what"]), js(doc["commit"]), js(doc["epilogues"]),
               wrapped(doc["blocks"], 1), wrapped(doc["plans"], 4), wrapped(doc["default"], 60), knobs))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="record again and compare with the committed fixture instead of writing it")
    args = ap.parse_args()
    doc = record_all()
    if args.check:
        with open(FIXTURE) as f:
            want = json.load(f)
        same = all(json.loads(json.dumps(doc[k])) == want[k] for k in ("epilogues", "blocks", "plans", "default", "knobs"))
        print(f"{len(doc['default'])} cases, {1 + len(doc['knobs'])} knob settings: {'identical to' if same else 'DIFFERENT from'} the fixture (recorded on {want['commit']})")
        sys.exit(0 if same else 1)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "nextgen-uia_amd/uia_hip/ops.py"], capture_output=True, text=True).stdout.strip()
    doc = dict(what="launches ops.gemm() made of each case on the commit named here (tools/record_gemm_launch_plans.py)", commit=commit + ("+modified ops.py" if dirty else ""), **doc)
    with open(FIXTURE, "w") as f:
        f.write(dumps(doc))
    assert json.loads(dumps(doc)) == json.loads(json.dumps(doc))
    print(f"{FIXTURE}: {len(doc['default'])} cases, {len(doc['plans'])} distinct plans, {os.path.getsize(FIXTURE)} bytes, commit {doc['commit']}")


if __name__ == "__main__":
    main()
