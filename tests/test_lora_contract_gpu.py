"""-m gpu: what the kernels that apply or regenerate the LoRA dropout must compute — uia_dropout, the N = 64 stream GEMM (tile cfg 16,
drop_where = 1), the K = 64 stream GEMM (tile cfg 23, drop_where = 2), the run-time GEMM epilogue, uia_wgrad / _ex / _drop / _group,
uia_lora_rank_update, uia_ln_lora_down — through their C entry points, at the small shapes where they branch: kept sets, dropped
operands and untouched elements bit for bit against the host restatement of the generator, products element-wise against the float64
restatements of tests/lora_reference.py on the operands the kernel sees.  Where the ops wrapper accepts the form, the same case runs
through it and must give the same bits (a weight gradient of more than one 512-row chunk meets in float atomics of no fixed order:
its wrapper run is held to the float64 bound instead).  The last test pins the three call sites of Mona's per-element generator to
the host mask.

Every output is a view into a larger NaN-filled buffer (tests/guarded_out.py).  Each test loops over its cases and fails once with
the collected list; its report prints the worst error/bound per bar."""
import ctypes as C

import pytest
import torch

import lora_reference as R
from guarded_out import Out, dev, guards

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DSEEDS = R.SEEDS[5:]                                            # the four seeds functional._next_seed derives for base 0x5EED


@pytest.fixture(scope="module")
def ops():
    from uia_hip import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


def to_dev(t, dt=None):
    return t.to(dt if dt is not None else t.dtype).to(dev())


def strided(t, ld):
    """t [rows, cols] on the device as a view of a NaN-filled [rows, ld] buffer (the kernel must not depend on the padding)."""
    if ld == t.shape[1]:
        return to_dev(t).contiguous()
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=dev())
    buf[:, :t.shape[1]] = to_dev(t)
    return buf[:, :t.shape[1]]


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def finish(ck):
    print(ck.report(limit=0))
    assert ck.ok(), ck.report()


def call(ops, name, *args):
    ops.check(getattr(ops.lib(), name)(ops._stream(), *args), name)


# ------------------------------------------------------------------------------------------ the generator: uia_dropout
def _dropout_cases():
    cases = [(n, p, s) for n in R.DROPOUT_N[:2] for p in R.DROPOUT_P for s in R.SEEDS]               # one group, 257 groups: every p with every seed
    n = R.DROPOUT_N[2]                                                                                # past one sweep of the grid: every p, every seed
    return cases + [(n, p, R.SEEDS[5]) for p in R.DROPOUT_P] + [(n, 0.25, s) for s in R.SEEDS if s != R.SEEDS[5]]


def test_dropout_equals_the_host_generator(ops):
    ck = R.Checker()
    src = {(dt, n): rnd(n, seed=n % 1000 + (dt == BF), scale=2.0).to(dt) for dt in (BF, F32) for n in R.DROPOUT_N}
    dst0 = {(dt, n): rnd(n, seed=n % 1000 + 7, scale=2.0).to(dt) for dt in (BF, F32) for n in R.DROPOUT_N}
    dsrc = {k: to_dev(v) for k, v in src.items()}
    for ci, (n, p, seed) in enumerate(_dropout_cases()):
        keep = R.keep_mask(seed, 1, n, p).reshape(-1)
        inv = torch.tensor(float(R.inv_keep32(p)), dtype=F32)
        if R.thresh16(p) == 0 and not bool(keep.all()):
            ck.fail("host mask", f"p={p}", "threshold 0 must keep every element")
        for dt in (BF, F32):
            ctx = f"{dt} n={n} p={p} seed={seed:#x}"
            code = ops._code(dt)
            # ones: the kept set, bit for bit (a kept one is fp32 1/(1-p) rounded to the dtype, a dropped one is +0)
            ones = Out((n,), dt)
            call(ops, "uia_dropout", code, n, ptr(torch.ones(n, dtype=dt, device=dev())), ptr(ones.t), p, seed, 0)
            ck.exact("dropout kept set", ones.t, torch.where(keep, inv, torch.zeros(())).to(dt), ctx)
            # random values, accumulate = 0 and 1
            for acc in (0, 1):
                out = Out((n,), dt, init=dst0[dt, n])
                call(ops, "uia_dropout", code, n, ptr(dsrc[dt, n]), ptr(out.t), p, seed, acc)
                want, _ = R.dropout(src[dt, n], p, seed, bool(acc), dst0[dt, n], keep=keep)
                ck.exact(f"dropout values accumulate={acc}", out.t, want, ctx)
                if ci % 4 == acc:                                   # the wrapper: the same bits
                    wo = Out((n,), dt, init=dst0[dt, n])
                    ops.dropout(dsrc[dt, n], wo.t, p, seed, accumulate=bool(acc))
                    ck.exact("dropout wrapper", wo.t, out.t, ctx)
                    guards(ck, "guards", ctx, wo)
                guards(ck, "guards", ctx, out)
            guards(ck, "guards", ctx, ones)
    finish(ck)


# ------------------------------------------------------------------------------------------ GEMM descriptors
def gemm_c(ops, tile_cfg, a, w, M, N, K, **f):
    d = ops.GemmDesc()
    d.A, d.lda, d.W, d.ldw, d.M, d.N, d.K, d.alpha = a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), M, N, K, f.pop("alpha", 1.0)
    for k, v in f.items():
        setattr(d, k, v.data_ptr() if torch.is_tensor(v) else v)
    call(ops, "uia_gemm", ops._code(a.dtype), C.byref(d), tile_cfg)


def test_n64_stream_gemm_drops_its_a_operand(ops):
    ck = R.Checker()
    ci = 0
    for M in R.GEMM_A_M:
        for K in R.GEMM_A_K:
            for with_out in (True, False):
                ci += 1
                p, seed = (0.1, 0.5)[ci % 2], DSEEDS[ci % 4]
                lda = K + 8 * (ci % 3 == 0)                             # the mask follows the logical width K, not lda
                ctx = f"M={M} K={K} lda={lda} p={p} a_drop_out={with_out} bias={ci % 2 == 0}"
                a, w = rnd(M, K, seed=M + K).to(BF), rnd(64, K, seed=K, scale=0.2).to(BF)
                bias = rnd(64, seed=3) if ci % 2 == 0 else None
                (t_ref, ad_ref), mag = R.gemm_drop_a(a, w, bias, p, seed)
                da, dw, db = strided(a, lda), to_dev(w), to_dev(bias) if bias is not None else None
                t = Out((M, 64), BF, ld=72)
                xd = Out((M, K), BF, ld=lda) if with_out else None
                f = dict(outT=t.t, ldo=72, drop_where=1, drop_p=p, drop_seed=seed)
                if bias is not None:
                    f["bias"] = db
                if with_out:
                    f["a_drop_out"] = xd.t
                gemm_c(ops, 16, da, dw, M, 64, K, **f)
                ck.check("gemm drop a: t", t.t, t_ref, R.bound(t_ref, mag, R.C_GEMM_DROP_A, BF), ctx)
                if with_out:
                    ck.exact("gemm drop a: a_drop_out", xd.t, ad_ref, ctx)
                t2 = Out((M, 64), BF, ld=72)
                xd2 = Out((M, K), BF, ld=lda) if with_out else None
                ops.gemm(da, dw, bias=db, out_t=t2.t, drop=("a", p, seed, xd2.t if with_out else None), tile_cfg=16)
                ck.exact("gemm drop a: wrapper t", t2.t, t.t, ctx)
                if with_out:
                    ck.exact("gemm drop a: wrapper a_drop_out", xd2.t, xd.t, ctx)
                guards(ck, "guards", ctx, *(o for o in (t, xd, t2, xd2) if o is not None))
    finish(ck)


def test_accumulator_dropout_k64_stream_and_runtime_epilogue(ops):
    ck = R.Checker()
    alpha = 1.75
    shapes = [(M, N, 64, 23) for M in R.GEMM_ACC_M for N in R.GEMM_ACC_N]
    Mt, Nt, Kt = R.GEMM_ACC_TILED
    plan = ops.plan_gemm(Mt, Nt, Kt, 2, ops.num_cus(0), 0, drop="acc", alpha=alpha, out_t=True, resid_t=True)
    assert len(plan) == 1 and plan[0].base == 3 and plan[0].tile_cfg & 255 == 0, plan      # a tiled kernel by the launcher's own choice: its run-time epilogue
    plan = ops.plan_gemm(Mt, Nt, Kt, 2, ops.num_cus(0), 0, drop="acc", alpha=alpha, out32=True, resid=True)
    assert len(plan) == 1 and plan[0].base == 3, plan
    shapes.append((Mt, Nt, Kt, 0))
    for ci, (M, N, K, cfg) in enumerate(shapes):
        p, seed = (0.1, 0.5)[ci % 2], DSEEDS[ci % 4]
        a, w = rnd(M, K, seed=M + N).to(BF), rnd(N, K, seed=N + 1, scale=0.3).to(BF)
        bias = rnd(N, seed=4) if ci % 2 else None
        resid = rnd(M, N, seed=5)
        da, dw, db = to_dev(a), to_dev(w), to_dev(bias) if bias is not None else None
        for form in ("bf16 in place", "fp32 out32 + resid"):
            ctx = f"M={M} N={N} K={K} cfg={cfg} p={p} bias={bias is not None} {form}"
            outs = []
            for via in ("c", "wrapper"):
                if form == "bf16 in place":
                    r0 = resid.to(BF)
                    o = Out((M, N), BF, ld=N + 8, init=r0)
                    if via == "c":
                        f = dict(alpha=alpha, residT=o.t, ldrT=N + 8, outT=o.t, ldo=N + 8, drop_where=2, drop_p=p, drop_seed=seed)
                        if bias is not None:
                            f["bias"] = db
                        gemm_c(ops, cfg, da, dw, M, N, K, **f)
                    else:
                        ops.gemm(da, dw, bias=db, alpha=alpha, resid_t=o.t, out_t=o.t, drop=("acc", p, seed), tile_cfg=cfg)
                    dt = BF
                else:
                    r0 = resid
                    dr = strided(resid, N + 4)
                    o = Out((M, N), F32, ld=N + 12)
                    if via == "c":
                        f = dict(alpha=alpha, resid=dr, ldr=N + 4, out32=o.t, ldo32=N + 12, drop_where=2, drop_p=p, drop_seed=seed)
                        if bias is not None:
                            f["bias"] = db
                        gemm_c(ops, cfg, da, dw, M, N, K, **f)
                    else:
                        ops.gemm(da, dw, bias=db, alpha=alpha, resid=dr, out32=o.t, drop=("acc", p, seed), tile_cfg=cfg)
                    dt = F32
                outs.append(o)
            ref, mag, keep = R.gemm_drop_acc(a, w, alpha, bias, p, seed, r0)
            bar = "drop acc cfg 23" if cfg == 23 else "drop acc run-time epilogue"
            ck.check(f"{bar} {form}", outs[0].t, ref, R.bound(ref, mag, R.C_GEMM_DROP_ACC, dt), ctx)
            ck.exact(f"{bar}: dropped elements keep the residual", outs[0].t.cpu()[~keep], r0[~keep], ctx)
            ck.exact(f"{bar}: wrapper", outs[1].t, outs[0].t, ctx)
            guards(ck, "guards", ctx, *outs)
    finish(ck)


# ------------------------------------------------------------------------------------------ weight gradients
def _wgrad_check(ck, bar, ctx, dw, db, r):
    """dw / db are exactly the valid extent ([i_valid, j_valid] rows ldw apart, [i_valid]): everything around them — the padding columns
    up to ldw, the rows and columns of the padded tile past the extent, the guards — must stay NaN."""
    ck.check(bar + " dW", dw.t, r["dw"], R.bound(r["dw"], r["mag_dw"], R.C_WGRAD), ctx)
    if db is not None:
        ck.check(bar + " dbias", db.t, r["db"], R.bound(r["db"], r["mag_db"], R.C_WGRAD_BIAS), ctx)
    guards(ck, "guards", ctx, dw, *([db] if db is not None else []))


def test_wgrad_every_form(ops):
    ck = R.Checker()
    ci = 0
    for M in R.WGRAD_M:
        for I, J in R.WGRAD_IJ:
            ci += 1
            one_chunk = M <= 512                                    # one atomic add per element: run-to-run identical bits
            for dt in (BF, F32):
                a, b = rnd(M, I, seed=M + I).to(dt), rnd(M, J, seed=M + J + 1).to(dt)
                code = ops._code(dt)
                # ---- plain: a dense [I, J] gradient and dbias, accumulated into non-zero buffers
                ctx = f"plain {dt} M={M} {I}x{J}"
                dw0, db0 = rnd(I, J, seed=1), rnd(I, seed=2)
                da, dbm = to_dev(a), to_dev(b)
                dw, db = Out((I, J), F32, init=dw0), Out((I,), F32, init=db0)
                call(ops, "uia_wgrad", code, M, I, J, ptr(da), I, ptr(dbm), J, 0.5, ptr(dw.t), ptr(db.t))
                r = R.wgrad(a, b, 0.5, dw0, dbias0=db0)
                _wgrad_check(ck, "wgrad", ctx, dw, db, r)
                dw2, db2 = Out((I, J), F32, init=dw0), Out((I,), F32, init=db0)
                ops.wgrad(da, dbm, dw2.t, db2.t, alpha=0.5)
                if one_chunk:
                    ck.exact("wgrad wrapper", dw2.t, dw.t, ctx)
                    ck.exact("wgrad wrapper dbias", db2.t, db.t, ctx)
                else:
                    _wgrad_check(ck, "wgrad wrapper", ctx, dw2, db2, r)
                # ---- ex: a valid extent inside the padded tile, ldw > j_valid, lda > I, ldb > J, dbias with i_valid < I
                name, (iv, jv) = R.WGRAD_VALID[1 + (ci + (dt == F32)) % 3]
                iv, jv = iv or I, jv or J
                lda, ldb, ldw = I + 8, J + 16, jv + 3
                ctx = f"ex {dt} M={M} {I}x{J} valid {iv}x{jv} lda={lda} ldb={ldb} ldw={ldw}"
                dw0, db0 = rnd(iv, jv, seed=3), rnd(iv, seed=4)
                da, dbm = strided(a, lda), strided(b, ldb)
                dw, db = Out((iv, jv), F32, ld=ldw, init=dw0), Out((iv,), F32, init=db0)
                call(ops, "uia_wgrad_ex", code, M, I, J, ptr(da), lda, ptr(dbm), ldb, 1.5, ptr(dw.t), ldw, iv, jv, ptr(db.t))
                r = R.wgrad(a, b, 1.5, dw0, iv, jv, dbias0=db0)
                _wgrad_check(ck, "wgrad_ex", ctx, dw, db, r)
                dw2, db2 = Out((iv, jv), F32, init=dw0), Out((iv,), F32, init=db0)
                ops.wgrad(da, dbm, dw2.t, db2.t, alpha=1.5)          # the wrapper's ldw is j_valid
                if one_chunk:
                    ck.exact("wgrad_ex wrapper", dw2.t, dw.t, ctx)
                    ck.exact("wgrad_ex wrapper dbias", db2.t, db.t, ctx)
                else:
                    _wgrad_check(ck, "wgrad_ex wrapper", ctx, dw2, db2, r)
            # ---- drop (bf16): the mask of a [M, drop_ld] tensor regenerated over the window of J columns at drop_col0
            a, b = rnd(M, I, seed=M + I).to(BF), rnd(M, J, seed=M + J + 1).to(BF)
            p, seed = (0.1, 0.5)[ci % 2], DSEEDS[ci % 4]
            for drop_ld, col0 in ((J, 0), (J + 64, 8), (J + 64, 64)):
                name, (iv, jv) = R.WGRAD_VALID[(ci + col0 // 8) % 4]
                iv, jv = iv or I, jv or J
                ldw = jv + (5 if col0 else 0)
                ctx = f"drop M={M} {I}x{J} valid {iv}x{jv} p={p} drop_ld={drop_ld} drop_col0={col0} ldw={ldw}"
                full = rnd(M, drop_ld, seed=M + J + col0).to(BF)
                full[:, col0:col0 + J] = b
                dfull = to_dev(full)
                da, dbm = to_dev(a), dfull[:, col0:col0 + J]
                keep = R.keep_mask(seed, M, J, p, ld=drop_ld, col0=col0)
                dw0 = rnd(iv, jv, seed=5)
                dw = Out((iv, jv), F32, ld=ldw, init=dw0)
                call(ops, "uia_wgrad_drop", ops._code(BF), M, I, J, ptr(da), I, ptr(dbm), drop_ld, 0.75, ptr(dw.t), ldw, iv, jv, p, seed, drop_ld, col0)
                r = R.wgrad(a, b, 0.75, dw0, iv, jv, drop=(p, keep))
                _wgrad_check(ck, "wgrad_drop", ctx, dw, None, r)
                if col0 == 0:                                       # the wrapper takes the whole dropped tensor only
                    dw2 = Out((iv, jv), F32, init=dw0)
                    ops.wgrad(da, dbm, dw2.t, alpha=0.75, drop=(p, seed))
                    if one_chunk:
                        ck.exact("wgrad_drop wrapper", dw2.t, dw.t, ctx)
                    else:
                        _wgrad_check(ck, "wgrad_drop wrapper", ctx, dw2, None, r)
            # ---- group: 1, 3 or 4 problems of one shape, each with its own seed; without dropout with dbias
            n = (1, 3, 4)[ci % 3]
            for with_drop in (False, True):
                name, (iv, jv) = R.WGRAD_VALID[(ci + with_drop) % 4]
                iv, jv = iv or I, jv or J
                drop_ld, col0 = (J + 64, 8) if (with_drop and ci % 2) else (J, 0)
                lda = I + 8 * (ci % 2)
                ldw = jv + 4 * (ci % 2)
                p = (0.5, 0.1)[ci % 2]
                ctx = f"group n={n} M={M} {I}x{J} valid {iv}x{jv} drop={with_drop} p={p} drop_ld={drop_ld} col0={col0} lda={lda} ldw={ldw}"
                As = [rnd(M, I, seed=M + I + g).to(BF) for g in range(n)]
                Bs = [rnd(M, J, seed=M + J + 10 + g).to(BF) for g in range(n)]
                dAs = [strided(x, lda) for x in As]
                fulls = [torch.zeros(M, drop_ld, dtype=BF, device=dev()) for _ in range(n)]
                for g in range(n):
                    fulls[g][:, col0:col0 + J] = to_dev(Bs[g])
                dBs = [x[:, col0:col0 + J] for x in fulls]
                dw0s = [rnd(iv, jv, seed=20 + g) for g in range(n)]
                db0s = [rnd(iv, seed=30 + g) for g in range(n)]
                dws = [Out((iv, jv), F32, ld=ldw, init=dw0s[g]) for g in range(n)]
                dbs = [Out((iv,), F32, init=db0s[g]) for g in range(n)] if not with_drop else [None] * n
                d = ops.WgradGroupDesc()
                d.n, d.M, d.I, d.J, d.lda, d.ldb, d.ldw, d.i_valid, d.j_valid, d.alpha = n, M, I, J, lda, drop_ld, ldw, iv, jv, 1.25
                for g in range(n):
                    d.A[g], d.B[g], d.dW[g] = dAs[g].data_ptr(), dBs[g].data_ptr(), dws[g].t.data_ptr()
                    if dbs[g] is not None and g != 1:               # problem 1 of a group without a bias gradient
                        d.dbias_A[g] = dbs[g].t.data_ptr()
                    d.drop_seed[g] = DSEEDS[g]
                if with_drop:
                    d.drop_p, d.drop_ld, d.drop_col0 = p, drop_ld, col0
                call(ops, "uia_wgrad_group", ops._code(BF), C.byref(d))
                rs = []
                for g in range(n):
                    has_b = dbs[g] is not None and g != 1
                    keep = R.keep_mask(DSEEDS[g], M, J, p, ld=drop_ld, col0=col0) if with_drop else None
                    r = R.wgrad(As[g], Bs[g], 1.25, dw0s[g], iv, jv, drop=(p, keep) if with_drop else None, dbias0=db0s[g] if has_b else None)
                    rs.append(r)
                    _wgrad_check(ck, "wgrad_group", f"{ctx} problem {g}", dws[g], dbs[g] if has_b else None, r)
                    if dbs[g] is not None and not has_b:
                        ck.exact("wgrad_group: no bias gradient asked", dbs[g].t, db0s[g], f"{ctx} problem {g}")
                if col0 == 0 and ldw == jv:                         # the wrapper: contiguous gradients, whole dropped tensors
                    dw2 = [Out((iv, jv), F32, init=dw0s[g]) for g in range(n)]
                    db2 = [Out((iv,), F32, init=db0s[g]) for g in range(n)] if not with_drop else None
                    ops.wgrad_group(dAs, dBs, [o.t for o in dw2], [o.t if g != 1 else None for g, o in enumerate(db2)] if db2 else None, alpha=1.25,
                                    drop=(p, list(DSEEDS[:n])) if with_drop else None)
                    for g in range(n):
                        if one_chunk:
                            ck.exact("wgrad_group wrapper", dw2[g].t, dws[g].t, f"{ctx} problem {g}")
                        else:
                            ck.check("wgrad_group wrapper dW", dw2[g].t, rs[g]["dw"], R.bound(rs[g]["dw"], rs[g]["mag_dw"], R.C_WGRAD), f"{ctx} problem {g}")
                    guards(ck, "guards", ctx, *dw2)
    finish(ck)


# ------------------------------------------------------------------------------------------ uia_lora_rank_update
def _rank_case(ops, ck, ctx, M, N, nsrc, p, ldo, ldw, ldq, q_gap, bar="lora_rank_update"):
    alpha = 1.5
    qs = [rnd(M, 64, seed=M + N + s).to(BF) for s in range(nsrc)]
    ws = [rnd(N, 64, seed=N + 10 + s, scale=0.3).to(BF) for s in range(nsrc)]
    out0 = rnd(M, N, seed=M + 3).to(BF)
    q_stride = M * ldq + q_gap
    qbuf = torch.full((nsrc * q_stride,), float("nan"), dtype=BF, device=dev())
    for s in range(nsrc):
        qbuf[s * q_stride:s * q_stride + M * ldq].view(M, ldq)[:, :64] = to_dev(qs[s])
    dws = [strided(w, ldw) for w in ws]
    out = Out((M, N), BF, ld=ldo, init=out0)
    d = ops.LoraRankDesc()
    d.M, d.N, d.nsrc, d.alpha = M, N, nsrc, alpha
    d.Q, d.ldq, d.q_stride = qbuf.data_ptr(), ldq, q_stride
    for s in range(nsrc):
        d.W[s] = dws[s].data_ptr()
        d.seed[s] = DSEEDS[s]
    d.ldw, d.out, d.ldo, d.drop_p = ldw, out.t.data_ptr(), ldo, p
    call(ops, "uia_lora_rank_update", ops._code(BF), C.byref(d))
    keeps = [R.keep_mask(DSEEDS[s], M, N, p) for s in range(nsrc)] if p > 0 else None
    ref, mag = R.lora_rank_update(out0, qs, ws, alpha, p, keeps)
    ck.check(bar, out.t, ref, R.bound(ref, mag, R.C_RANK, BF), ctx)
    if p > 0:
        none = ~torch.stack(keeps).any(0)                           # every source drops the position: the output keeps its bits
        ck.exact(bar + ": all sources dropped", out.t.cpu()[none], out0[none], ctx)
    if ldq == 64 and q_gap == 0:                                    # the wrapper takes contiguous sources
        out2 = Out((M, N), BF, ld=ldo, init=out0)
        ops.lora_rank_update(qbuf.view(nsrc, M, 64), dws, out2.t, alpha, p, list(DSEEDS[:nsrc]))
        ck.exact(bar + " wrapper", out2.t, out.t, ctx)
        guards(ck, "guards", ctx, out2)
    guards(ck, "guards", ctx, out)


def test_lora_rank_update_small_shapes(ops):
    ck = R.Checker()
    ci = 0
    for nsrc in (1, 2, 3):
        for N in R.RANK_N:
            for M in R.RANK_M:
                ci += 1
                p = (0.0, 0.25)[ci % 2]
                ldo, ldw = N + 8 * (ci % 3 == 0), 64 + 8 * (ci % 3 == 1)
                ldq, q_gap = (72, 64) if ci % 4 == 3 else (64, 0)
                _rank_case(ops, ck, f"nsrc={nsrc} N={N} M={M} p={p} ldo={ldo} ldw={ldw} ldq={ldq} q_stride=M*ldq+{q_gap}", M, N, nsrc, p, ldo, ldw, ldq, q_gap)
    finish(ck)


def test_lora_rank_update_waves_walk_two_three_four_units(ops):
    """N = 1024 on this device's CU count: the smallest M at which some wave walks 2, 3 and 4 units through the three register sets
    (2049, 4097 and 6145 rows at 256 CUs: tests/lora_reference.rank_walk_rows)."""
    ck = R.Checker()
    ncu = ops.num_cus(0)
    for k, (nsrc, p) in zip((2, 3, 4), ((3, 0.25), (2, 0.0), (3, 0.25))):
        M = R.rank_walk_rows(ncu, 1024, k)
        _rank_case(ops, ck, f"{k} units: nsrc={nsrc} N=1024 M={M} p={p} ncu={ncu}", M, 1024, nsrc, p, 1024 + 8 * (k == 3), 64, 64, 0, bar=f"lora_rank_update {k} units")
    finish(ck)


# ------------------------------------------------------------------------------------------ uia_ln_lora_down
def _ln_launch(ops, x_dev, ldx, M, D, gamma, beta, eps, a_devs, nsrc, p, t_gap=0):
    h = Out((M, D), BF)
    t_stride = M * 64 + t_gap
    t = Out((nsrc, t_stride), BF)
    d = ops.LnLoraDesc()
    d.M, d.D, d.nsrc, d.eps = M, D, nsrc, eps
    d.x, d.ldx, d.gamma, d.beta, d.h = x_dev.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), h.t.data_ptr()
    for s in range(nsrc):
        d.A[s] = a_devs[s].data_ptr()
        d.seed[s] = DSEEDS[s]
    d.lda, d.T, d.t_stride, d.drop_p = a_devs[0].stride(0), t.t.data_ptr(), t_stride, p
    call(ops, "uia_ln_lora_down", ops._code(BF), C.byref(d))
    return h, t


def _ln_judge(ck, bar, ctx, h, t, M, D, nsrc, rank, p, href, hmag, a_rows, t_gap=0):
    ck.check(bar + " h", h.t, href, R.bound(href, hmag, R.C_LN_H, BF), ctx)
    hk = h.t.cpu()
    tk = t.t.cpu()
    for s in range(nsrc):
        hd = R.dropped(hk, p, R.keep_mask(DSEEDS[s], M, D, p)) if p > 0 else hk
        a64 = a_rows[s][:rank].to(R.F64)
        ts = tk[s, :M * 64].view(M, 64)
        ref, mag = hd.to(R.F64) @ a64.T, hd.to(R.F64).abs() @ a64.abs().T
        ck.check(bar + " t", ts[:, :rank], ref, R.bound(ref, mag, R.C_LN_T, BF), f"{ctx} source {s}")
        ck.exact(bar + " t columns past the rank are zero", ts[:, rank:], torch.zeros(M, 64 - rank, dtype=BF), f"{ctx} source {s}")
        if t_gap:
            ck.exact(bar + " gap between the sources untouched", tk[s, M * 64:], torch.full((t_gap,), float("nan"), dtype=BF), f"{ctx} source {s}")
    guards(ck, "guards", ctx, h, t)


def _ln_operands(D, nsrc, rank, seed):
    gamma, beta = rnd(D, seed=seed, scale=0.5, shift=1.0), rnd(D, seed=seed + 1, scale=0.3)
    a_rows = []
    for s in range(nsrc):
        a = torch.zeros(16, D, dtype=BF)                            # rank rows, zero-padded to the 16 the kernel reads
        a[:rank] = rnd(rank, D, seed=seed + 2 + s, scale=0.2).to(BF)
        a_rows.append(a)
    return gamma, beta, a_rows


def test_ln_lora_down_small_shapes(ops):
    ck = R.Checker()
    eps = float(torch.tensor(1e-5, dtype=F32))
    ci = 0
    for D in R.LN_D:
        for M in R.LN_M:
            combos = [(n, r) for n in (1, 2, 3) for r in R.LN_RANK] if M == 17 else [((ci + M) % 3 + 1, R.LN_RANK[(ci + M // 2) % 3]), (3 - (ci + M) % 3, R.LN_RANK[(ci + M // 2 + 1) % 3])]
            for nsrc, rank in combos:
                ci += 1
                p = (0.0, 0.1)[ci % 2]
                ldx = D + 4 * (ci % 3 == 0)
                shift = 100.0 if (M == 100 and ci % 2) or (M == 17 and nsrc == 2 and rank == 8) else 0.5       # rows with a mean of about 100
                t_gap = 64 * (ci % 4 == 1)
                ctx = f"D={D} M={M} nsrc={nsrc} rank={rank} p={p} ldx={ldx} mean~{shift} t_stride=64M+{t_gap}"
                x = rnd(M, D, seed=M + D + ci, scale=1.5, shift=shift)
                gamma, beta, a_rows = _ln_operands(D, nsrc, rank, ci)
                h, t = _ln_launch(ops, strided(x, ldx), ldx, M, D, to_dev(gamma), to_dev(beta), eps, [to_dev(a) for a in a_rows], nsrc, p, t_gap)
                href, hmag = R.layernorm(x, gamma, beta, eps)
                _ln_judge(ck, "ln_lora_down", ctx, h, t, M, D, nsrc, rank, p, href, hmag, a_rows, t_gap)
                if ldx == D and t_gap == 0:                          # the wrapper: contiguous x rows, sources back to back
                    h2, t2 = Out((M, D), BF), Out((nsrc, M, 64), BF)
                    ops.ln_lora_down(to_dev(x), to_dev(gamma), to_dev(beta), eps, h2.t, [to_dev(a) for a in a_rows], t2.t, p, list(DSEEDS[:nsrc]))
                    ck.exact("ln_lora_down wrapper h", h2.t, h.t, ctx)
                    ck.exact("ln_lora_down wrapper t", t2.t, t.t.cpu()[:, :M * 64], ctx)
                    guards(ck, "guards", ctx, h2, t2)
    finish(ck)


def test_ln_lora_down_more_tiles_than_blocks(ops):
    """The launch has min(tiles, per_cu·ncu) workgroups, per_cu from the occupancy query on 256 threads and the kernel's LDS.  With D = 1024
    and three sources a workgroup holds 16·2064 + 3·4096 = 45 312 bytes, so per_cu is 1, 2 or 3 whatever the register count: the smallest M
    with more 16-row tiles than blocks is 16·per_cu·ncu + 1, i.e. one of 4097, 8193, 12 289 at 256 CUs.  All three run; the float64
    LayerNorm is taken once on the longest and shared (rows are independent)."""
    ck = R.Checker()
    eps = float(torch.tensor(1e-5, dtype=F32))
    D, nsrc, rank, p = 1024, 3, 16, 0.1
    ncu = ops.num_cus(0)
    Ms = [R.ln_tiles_rows(ncu, per_cu) for per_cu in (1, 2, 3)]
    x = rnd(Ms[-1], D, seed=9, scale=1.5, shift=0.5)
    gamma, beta, a_rows = _ln_operands(D, nsrc, rank, 5)
    href, hmag = R.layernorm(x, gamma, beta, eps)
    dx, dg, db, das = to_dev(x), to_dev(gamma), to_dev(beta), [to_dev(a) for a in a_rows]
    for M in Ms:
        h, t = _ln_launch(ops, dx, D, M, D, dg, db, eps, das, nsrc, p)
        _ln_judge(ck, "ln_lora_down tiles > blocks", f"D={D} M={M} nsrc={nsrc} p={p} ncu={ncu}", h, t, M, D, nsrc, rank, p, href[:M], hmag[:M], a_rows)
    finish(ck)


# ------------------------------------------------------------------------------------------ Mona's per-element generator
def test_mona_seeded_launches_equal_the_host_mask(ops):
    """A seeded launch against the same launch given the host keep_mask, bit for bit: the spatial forward, the spatial backward and the
    fused forward index the generator with the flat element index of d [B, 1 + h·w, 64].  4 x 4 tokens: the smallest grid on which both
    the spatial kernels and the fused forward are exercised elsewhere in the suite."""
    ck = R.Checker()
    B, h, w, D = 2, 4, 4, 128
    Ntok = 1 + h * w
    P = dict(conv1_w=rnd(64, 9, seed=1, scale=0.2), conv1_b=rnd(64, seed=2, scale=0.1), conv2_w=rnd(64, 25, seed=3, scale=0.1), conv2_b=rnd(64, seed=4, scale=0.1),
             conv3_w=rnd(64, 49, seed=5, scale=0.05), conv3_b=rnd(64, seed=6, scale=0.1), proj_w=rnd(64, 64, seed=7, scale=0.2), proj_b=rnd(64, seed=8, scale=0.1))
    P = {k: to_dev(v) for k, v in P.items()}
    tt, dd = rnd(B, Ntok, 64, seed=9), rnd(B, Ntok, 64, seed=10)
    x = to_dev(rnd(B, Ntok, D, seed=11, scale=1.5))
    vec = lambda s, sh=1.0: to_dev(rnd(D, seed=s, scale=0.3, shift=sh))          # noqa: E731
    nw, nb, gm, gx, b2 = vec(12), vec(13, 0.0), vec(14, 0.0), vec(15), vec(16, 0.0)
    w1, w2, b1 = to_dev(rnd(64, D, seed=17, scale=0.1), BF), to_dev(rnd(D, 64, seed=18, scale=0.1), BF), to_dev(rnd(64, seed=19, scale=0.1))
    for p, seed in ((0.1, DSEEDS[0]), (0.5, DSEEDS[1]), (0.5, R.SEEDS[4])):
        mask = to_dev(R.mona_keep_mask(seed, (B, Ntok, 64), p))
        kept = float(mask.float().mean())
        if abs(kept - (1 - p)) > 5 * (p * (1 - p) / mask.numel()) ** 0.5:
            ck.fail("host mask", f"p={p}", f"keep rate {kept}")
        for dt in (BF, F32):
            ctx = f"{dt} p={p} seed={seed:#x}"
            t = to_dev(tt, dt)
            outs = []
            for kw in (dict(seed=seed), dict(keep_mask=mask)):
                d = Out((B, Ntok, 64), dt)
                ops.mona_spatial_fwd("baseline", B, h, w, t, P, d.t, p_drop=p, **kw)
                outs.append(d)
            ck.exact("mona_spatial_fwd seeded = host mask", outs[0].t, outs[1].t, ctx)
            zero = (outs[0].t == 0).cpu()
            ck.exact("mona_spatial_fwd zeros are the dropped elements", zero | mask.cpu().bool(), torch.ones_like(zero), ctx)
            guards(ck, "guards", ctx, *outs)
            runs = []
            for kw in (dict(seed=seed), dict(keep_mask=mask)):
                dtt = Out((B, Ntok, 64), dt)
                grads = {k: torch.zeros_like(v) for k, v in P.items()}
                ops.mona_spatial_bwd("baseline", B, h, w, t, P, to_dev(dd, dt), dtt.t, grads, p_drop=p, **kw)
                runs.append((dtt, grads))
            ck.exact("mona_spatial_bwd seeded = host mask", runs[0][0].t, runs[1][0].t, ctx)     # dt: every element written once, no atomics
            guards(ck, "guards", ctx, runs[0][0], runs[1][0])
        ctx = f"fused p={p} seed={seed:#x}"
        outs = []
        for kw in (dict(seed=seed), dict(keep_mask=mask)):
            y, d = Out((B, Ntok, D), F32), Out((B * Ntok, 64), BF)
            ops.mona_fused_fwd("baseline", B, h, w, x, nw, nb, gm, gx, w1, b1, w2, b2, P, y.t, d_out=d.t, p_drop=p, **kw)
            outs.append((y, d))
        ck.exact("mona_fused_fwd seeded = host mask: y", outs[0][0].t, outs[1][0].t, ctx)
        ck.exact("mona_fused_fwd seeded = host mask: d", outs[0][1].t, outs[1][1].t, ctx)
        zero = (outs[0][1].t == 0).cpu().reshape(B, Ntok, 64)
        ck.exact("mona_fused_fwd zeros are the dropped elements", zero | mask.cpu().bool(), torch.ones_like(zero), ctx)
        guards(ck, "guards", ctx, *outs[0], *outs[1])
    finish(ck)
