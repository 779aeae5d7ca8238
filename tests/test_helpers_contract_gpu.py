"""-m gpu: what the small kernels of csrc/decoder.hip, csrc/heads.hip and csrc/elementwise.hip must compute, through their wrappers
in uia_hip/ops.py, at the shapes where they branch: data movement bit-exact against torch's own rounding, elementwise and reductions
element-wise against the float64 restatements of tests/helpers_reference.py, on the operands the kernel sees.

Every output is a view into a larger NaN-filled buffer: an element the kernel does not write fails its comparison, and a write
outside the view (the guard regions, the padding columns of a strided view) fails the test.  Each test loops over its cases and
collects every failure (bar, case, worst flat index, error/bound) before it fails once with the list."""
import pytest
import torch

import helpers_reference as R
from guarded_out import PAD, Out, dev, guards

pytestmark = pytest.mark.gpu

DT = (torch.bfloat16, torch.float32)
# threads of one sweep of each file's capped grid-stride launches: 4096 blocks (decoder.hip), 2048 (elementwise.hip), 16384 (heads.hip)
SWEEP_DECODER, SWEEP_ELEMENTWISE, SWEEP_HEADS = 4096 * 256, 2048 * 256, 16384 * 256


@pytest.fixture(scope="module")
def ops():
    from uia_hip import ops as o
    return o


@pytest.fixture(scope="module")
def UiaError():
    from uia_hip._lib import UiaError as E
    return E


def rnd(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


def to_dev(t, dt=None):
    return t.to(dt if dt is not None else t.dtype).to(dev())


def finish(ck):
    assert ck.ok(), ck.report()


# ------------------------------------------------------------------------------------------ 3×3 patches
GRIDS = ((1, 1), (1, 7), (7, 1), (3, 5), (22, 22))


def test_im2col3x3_exact_and_col2im3x3_bounded(ops):
    ck = R.Checker()
    B = 2
    for dt in DT:
        for h, w in GRIDS:
            for tok_off in (0, 1, 2):
                for C in (4, 64, 68):
                    ctx = f"{dt} h={h} w={w} tok_off={tok_off} C={C}"
                    ntok = tok_off + h * w + 2                       # two tokens past the grid: neither read nor given a gradient
                    x = rnd(B, ntok, C, seed=h * 100 + w * 10 + C + tok_off)
                    cols = Out((B * h * w, 9 * C), dt)
                    ops.im2col3x3(to_dev(x), cols.t, h, w, tok_off=tok_off)
                    ck.exact("im2col3x3", cols.t, R.im2col3x3(x, h, w, tok_off).to(dt), ctx)
                    dcols = rnd(B * h * w, 9 * C, seed=7 + C).to(dt)
                    outs = []
                    for _ in range(2):
                        dx = Out((B, ntok, C), torch.float32)
                        ops.col2im3x3(to_dev(dcols), dx.t, h, w, tok_off=tok_off)
                        outs.append(dx)
                    ref = R.col2im3x3(dcols.double(), B, h, w, C, ntok, tok_off)
                    mag = R.col2im3x3_mag(dcols.double(), B, h, w, C, ntok, tok_off)
                    ck.check("col2im3x3", outs[0].t, ref, R.bound(ref, mag, R.C_COL2IM), ctx)
                    ck.exact("col2im3x3 deterministic", outs[1].t, outs[0].t, ctx)
                    guards(ck, "guards", ctx, cols, *outs)
    # past the 4096-block cap (one thread per float4): im2col3x3 with B·h·w·9·C / 4 threads, col2im3x3 with B·ntok·C / 4
    for B, h, w, C, which in ((8, 22, 22, 128, "im2col3x3"), (2, 22, 22, 4352, "col2im3x3")):
        ctx = f"bf16 B={B} h={h} w={w} C={C} past the grid cap"
        ntok = 1 + h * w + 2
        if which == "im2col3x3":
            assert B * h * w * 9 * C // 4 > SWEEP_DECODER
            x = rnd(B, ntok, C, seed=5)
            cols = Out((B * h * w, 9 * C), torch.bfloat16)
            ops.im2col3x3(to_dev(x), cols.t, h, w, tok_off=1)
            ck.exact("im2col3x3", cols.t, R.im2col3x3(x, h, w, 1).to(torch.bfloat16), ctx)
            guards(ck, "guards", ctx, cols)
        else:
            assert B * ntok * C // 4 > SWEEP_DECODER
            dcols = rnd(B * h * w, 9 * C, seed=6).to(torch.bfloat16)
            dx = Out((B, ntok, C), torch.float32)
            ops.col2im3x3(to_dev(dcols), dx.t, h, w, tok_off=1)
            ref = R.col2im3x3(dcols.double(), B, h, w, C, ntok, 1)
            ck.check("col2im3x3", dx.t, ref, R.bound(ref, R.col2im3x3_mag(dcols.double(), B, h, w, C, ntok, 1), R.C_COL2IM), ctx)
            guards(ck, "guards", ctx, dx)
    finish(ck)


# ------------------------------------------------------------------------------------------ pixel (un)shuffle
def test_unshuffle_shuffle_exact(ops):
    ck = R.Checker()
    B, h, w = 2, 3, 2
    bias = float(torch.tensor(0.3, dtype=torch.float32))
    for dt in DT:
        for k1, k2 in ((4, 4), (1, 4), (4, 1), (2, 3)):
            for ld in (k2 * k2, k2 * k2 + 5):
                ctx = f"{dt} k1={k1} k2={k2} ld={ld}"
                rows, H, W = B * h * w * k1 * k1, h * k1 * k2, w * k1 * k2
                tmp = rnd(rows, ld, seed=k1 * 10 + k2).to(dt)
                out = Out((B, H, W), torch.float32)
                ops.unshuffle(to_dev(tmp)[:, :k2 * k2] if ld > k2 * k2 else to_dev(tmp), out.t, B, h, w, k1, k2, bias=bias)
                ck.exact("unshuffle", out.t, R.unshuffle(tmp.float(), B, h, w, k1, k2) + torch.tensor(bias), ctx)
                dout = rnd(B, H, W, seed=k1 + k2)
                dtmp = Out((rows, ld), dt)
                ops.shuffle(to_dev(dout), dtmp.t, B, h, w, k1, k2)
                ck.exact("shuffle (padding columns zero)", dtmp.t, R.shuffle(dout, B, h, w, k1, k2, ld).to(dt), ctx)
                guards(ck, "guards", ctx, out, dtmp)
    B, h, w, k1, k2 = 65, 16, 16, 4, 4                      # one thread per k2 columns: past the 4096-block cap
    assert B * h * w * k1 * k1 * k2 > SWEEP_DECODER
    rows, H, W = B * h * w * k1 * k1, h * k1 * k2, w * k1 * k2
    ctx = f"bf16 B={B} {h}x{w} k1={k1} k2={k2} past the grid cap"
    tmp = rnd(rows, k2 * k2, seed=3).to(torch.bfloat16)
    out = Out((B, H, W), torch.float32)
    ops.unshuffle(to_dev(tmp), out.t, B, h, w, k1, k2, bias=bias)
    ck.exact("unshuffle", out.t, R.unshuffle(tmp.float(), B, h, w, k1, k2) + torch.tensor(bias), ctx)
    dout = rnd(B, H, W, seed=4)
    dtmp = Out((rows, k2 * k2), torch.bfloat16)
    ops.shuffle(to_dev(dout), dtmp.t, B, h, w, k1, k2)
    ck.exact("shuffle (padding columns zero)", dtmp.t, R.shuffle(dout, B, h, w, k1, k2, k2 * k2).to(torch.bfloat16), ctx)
    guards(ck, "guards", ctx, out, dtmp)
    finish(ck)


# ------------------------------------------------------------------------------------------ layout kernels of elementwise.hip
def test_layout_kernels_exact(ops):
    ck = R.Checker()
    cap = 2048 * 256 * 4                                    # cast: elements the capped grid covers in one sweep
    for dt in DT:
        for n in (4, cap - 4, cap, cap + 4):
            for scale in (1.0, float(torch.tensor(0.1, dtype=torch.float32))):
                src = rnd(n, seed=n % 97)
                out = Out((n,), dt)
                ops.cast(to_dev(src), out.t, scale)
                ck.exact("cast", out.t, (src * scale).to(dt), f"{dt} n={n} scale={scale}")
                guards(ck, "guards", f"cast {dt} n={n}", out)
        for rows, cols in ((1, 37), (37, 1), (33, 65), (70, 130), (1, 1)):
            src = rnd(rows, cols, seed=rows + cols)
            out = Out((cols, rows), dt)
            ops.transpose_cast(to_dev(src), out.t)
            ck.exact("transpose_cast", out.t, src.T.contiguous().to(dt), f"{dt} {rows}x{cols}")
            guards(ck, "guards", f"transpose_cast {dt} {rows}x{cols}", out)
        # the last two pass the 2048-block cap: the vectorised path (a float4 per thread), the padded path (an element per thread)
        for Bi, P, Hh, Ww, ldo in ((2, 16, 32, 48, None), (2, 32, 64, 32, None), (2, 14, 28, 42, 3 * 14 * 14 + 20), (2, 14, 14, 14, None),
                                   (16, 16, 224, 224, None), (4, 14, 224, 224, 640)):
            img = rnd(Bi, 3, Hh, Ww, seed=P)
            K = 3 * P * P
            out = Out((Bi * (Hh // P) * (Ww // P), ldo or K), dt)
            ops.im2col(to_dev(img), out.t, P)
            ck.exact("im2col", out.t, R.im2col(img, P, ldo).to(dt), f"{dt} B={Bi} P={P} ldo={ldo}")
            guards(ck, "guards", f"im2col {dt} P={P}", out)
    B, N, D = 3, 5, 68
    x0, cls, pos0 = rnd(B, N, D, seed=1), rnd(D, seed=2), rnd(D, seed=3)
    for p0 in (pos0, None):
        x = Out((B, N, D), torch.float32, init=x0)
        ops.fill_cls(x.t, to_dev(cls), to_dev(p0) if p0 is not None else None)
        want = x0.clone()
        want[:, 0] = cls + (p0 if p0 is not None else 0)
        ck.exact("fill_cls", x.t, want, f"pos0={p0 is not None}")
        guards(ck, "guards", "fill_cls", x)
    V, L, D = 50, 9, 68
    table, pos, typ = rnd(V, D, seed=4), rnd(L + 2, D, seed=5), rnd(D, seed=6)
    ids = torch.randint(0, V, (3, L), generator=torch.Generator().manual_seed(7))
    ids[0, 3], ids[1, 0], ids[2, L - 1] = -1, V, V + 100                 # outside the table: NaN rows, the table is not read
    for t0 in (typ, None):
        out = Out((3 * L, D), torch.float32)
        ops.embed(to_dev(ids), to_dev(table), to_dev(pos), to_dev(t0) if t0 is not None else None, out.t)
        ck.exact("embed", out.t, R.embed(ids.reshape(-1), torch.arange(L).repeat(3), table, pos, t0), f"type0={t0 is not None}")
        pidx = torch.tensor([0, 1, 2, L + 1, -1, L + 2, 4, 3, 0, 5, 6])
        pid = torch.tensor([1, 2, 3, 4, 5, 6, -3, V, 7, 8, 49])
        out = Out((pid.numel(), D), torch.float32)
        ops.embed_packed(to_dev(pid), to_dev(pidx), to_dev(table), to_dev(pos), to_dev(t0) if t0 is not None else None, out.t)
        ck.exact("embed_packed", out.t, R.embed(pid, pidx, table, pos, t0), f"type0={t0 is not None}")
        guards(ck, "guards", "embed", out)
    Bw, Dw = 300, 800                                       # rows·D / 4 threads past the 2048-block cap
    assert Bw * L * Dw // 4 > SWEEP_ELEMENTWISE
    tw, pw, yw = rnd(V, Dw, seed=14), rnd(L, Dw, seed=15), rnd(Dw, seed=16)
    idw = torch.randint(-2, V + 2, (Bw, L), generator=torch.Generator().manual_seed(17))
    out = Out((Bw * L, Dw), torch.float32)
    ops.embed(to_dev(idw), to_dev(tw), to_dev(pw), to_dev(yw), out.t)
    ck.exact("embed", out.t, R.embed(idw.reshape(-1), torch.arange(L).repeat(Bw), tw, pw, yw), "past the grid cap")
    guards(ck, "guards", "embed past the grid cap", out)
    pidw = torch.randint(-1, L + 1, (Bw * L,), generator=torch.Generator().manual_seed(18))
    out = Out((Bw * L, Dw), torch.float32)
    ops.embed_packed(to_dev(idw.reshape(-1)), to_dev(pidw), to_dev(tw), to_dev(pw), None, out.t)
    ck.exact("embed_packed", out.t, R.embed(idw.reshape(-1), pidw, tw, pw, None), "past the grid cap")
    guards(ck, "guards", "embed_packed past the grid cap", out)
    for src, idx in ((rnd(20, D, seed=8), torch.tensor([19, 0, 7, 7, 3, 19, 1])),
                     (rnd(50, Dw, seed=9), torch.randint(0, 50, (Bw * L,), generator=torch.Generator().manual_seed(19)))):
        out = Out((idx.numel(), src.shape[1]), torch.float32)
        ops.gather_rows(to_dev(src), to_dev(idx), out.t)
        ck.exact("gather_rows", out.t, src[idx], f"in-range, {idx.numel()} x {src.shape[1]}")
        guards(ck, "guards", "gather_rows", out)
    # the last one passes the 16384-block cap (an element per thread)
    for B, n, C, ld in ((2, 1, 5, 5), (3, 50, 1, 1), (2, 49, 300, 307), (4, 7, 64, 64), (64, 196, 352, 352)):
        dout = rnd(B, C, seed=B * n + C)
        dx = Out((B * n, C), torch.float32, ld=ld)
        ops.segment_mean(to_dev(dout), B, n, dx.t, backward=True)
        s = torch.tensor(1.0, dtype=torch.float32) / n
        ck.exact("segment_mean backward", dx.t, (s * dout).repeat_interleave(n, 0), f"B={B} n={n} C={C} ld={ld}")
        guards(ck, "guards", "segment_mean backward", dx)
    finish(ck)


def test_pack_weights_exact(ops):
    ck = R.Checker()
    for dt in DT:
        g = 64 // torch.tensor([], dtype=dt).element_size()
        # the K-blocked forms fill whole 64-byte groups: their padded extents are multiples of g (pack_table refuses anything else)
        # the last has more elements than the 256 x-blocks cover in one sweep of ~4 per thread
        for (Rr, Cc), pad, scale in (((37, 45), (64, 64), 0.5), ((32, 64), None, 1.0), ((1, 3), (32, 96), 3.0), ((520, 512), (544, 512), 0.25)):
            src = rnd(Rr, Cc, seed=Rr + Cc)
            RP, CP = pad if pad else (Rr, Cc)
            dests = {k: Out((RP * CP,), dt) for k in ("row", "row_kb", "tr", "tr_kb")}
            ent = (to_dev(src), dests["row"].t, dests["row_kb"].t, dests["tr"].t, dests["tr_kb"].t) + (((RP, CP, scale),) if pad or scale != 1 else ())
            table, n, mx = ops.pack_table([ent], dev())
            ops.pack_weights(table, n, mx, dt)
            want = R.pack_weights(src, scale, RP, CP, g, dt)
            for k, o in dests.items():
                ck.exact(f"pack_weights {k}", o.t, want[k], f"{dt} {Rr}x{Cc} pad={pad} scale={scale}")
                guards(ck, "guards", f"pack_weights {k}", o)
    finish(ck)


# ------------------------------------------------------------------------------------------ act_bwd
SPECIAL = torch.tensor([0.0, 1e-3, -1e-3, 4.0, -4.0, 30.0, -30.0, 100.0, -100.0, 1.0, -1.0])


def test_act_bwd_every_path(ops):
    ck = R.Checker()
    for dt in DT:
        # (n, element offset of y, element offset of out): the vector path, the scalar path by length, by pointer, and both paths
        # past the 4096-block cap (the vector path covers 8 elements per thread)
        for n, oy, oo in ((4096, 0, 0), (4099, 0, 0), (4100, 0, 0), (4096, 1, 0), (4096, 0, 1), (1 + 13, 0, 0), ((1 << 20) + 13, 0, 0),
                          ((1 << 23) + 64, 0, 0)):
            x = rnd(n, seed=n, scale=3.0)
            k = min(n, SPECIAL.numel())
            x[:k] = SPECIAL[:k]
            x[n - k:] = SPECIAL[:k]                                       # the tail too: the scalar path's last elements
            x = x.to(dt)
            dy = rnd(n, seed=n + 1).to(dt)
            for act in ("none", "relu", "gelu", "quick_gelu"):
                ctx = f"{dt} n={n} y offset {oy} out offset {oo} {act}"
                ybuf = torch.full((n + 8,), float("nan"), dtype=dt, device=dev())
                yv = x.clamp_min(0) if act == "relu" else x                 # ReLU's operand is the post-activation (zeros included)
                ybuf[oy:oy + n] = to_dev(yv)
                out = Out((n,), dt, offset=PAD + oo)
                ops.act_bwd(to_dev(dy), ybuf[oy:oy + n], act, out.t)
                ref = R.act_bwd(dy.double(), yv.double(), act)
                if act in ("none", "relu"):
                    ck.exact(f"act_bwd {act}", out.t, ref.to(dt), ctx)
                else:
                    c = R.C_ACT_GELU if act == "gelu" else R.C_ACT_QUICK
                    ck.check(f"act_bwd {act} {dt}", out.t, ref, R.bound(ref, R.act_bwd_mag(dy, yv, act), c, dt), ctx)
                guards(ck, "guards", ctx, out)
    finish(ck)


# ------------------------------------------------------------------------------------------ reductions
def test_layernorm_bwd_affine(ops):
    ck = R.Checker()
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    for dt in DT:
        for di, D in enumerate((4, 252, 256, 260, 768, 772, 1024)):
            for M in (1, 3, 4, 5, 4099):
                for with_res in ((False, True) if M in (3, 4099) else (bool((di + M) % 2),)):
                    ctx = f"{dt} D={D} M={M} dres={with_res}"
                    x = rnd(M, D, seed=D + M, scale=2.0, shift=3.0)
                    dy = rnd(M, D, seed=D * M + 1).to(dt)
                    gamma = rnd(D, seed=D, scale=0.5, shift=1.0)
                    dres = rnd(M, D, seed=D + 2 * M) if with_res else None
                    g0, b0 = rnd(D, seed=11), rnd(D, seed=12)
                    dx = Out((M, D), torch.float32)
                    gg, gb = Out((D,), torch.float32, init=g0), Out((D,), torch.float32, init=b0)
                    ops.layernorm_bwd_affine(to_dev(dy), to_dev(x), to_dev(gamma), eps, dx.t, gg.t, gb.t, dres=to_dev(dres) if with_res else None)
                    r = R.ln_affine_bwd(dy.double(), x.double(), gamma.double(), eps, dres.double() if with_res else None)
                    ck.check("ln_affine_bwd dx", dx.t, r["dx"], R.bound(r["dx"], r["mag_dx"], R.C_LN), ctx)
                    ref_g, ref_b = g0.double() + r["dg"], b0.double() + r["db"]           # the kernel ADDS into g_gamma / g_beta
                    ck.check("ln_affine_bwd dgamma", gg.t, ref_g, R.bound(ref_g, r["mag_dg"] + g0.double().abs(), R.C_LN), ctx)
                    ck.check("ln_affine_bwd dbeta", gb.t, ref_b, R.bound(ref_b, r["mag_db"] + b0.double().abs(), R.C_LN), ctx)
                    guards(ck, "guards", ctx, dx, gg, gb)
    finish(ck)


def test_film_fwd_bwd(ops):
    ck = R.Checker()
    B = 3
    for C in (1, 2, 4, 64, 256, 512):
        for N in (1, 7, 50):
            ctx = f"C={C} N={N}"
            x, mul, add, dy = rnd(B, N, C, seed=C + N), rnd(B, C, seed=C), rnd(B, C, seed=C + 1), rnd(B, N, C, seed=C * N)
            if C % 4 == 0:
                y = Out((B, N, C), torch.float32)
                ops.film_fwd(to_dev(x), to_dev(mul), to_dev(add), y.t)
                ref, mag = R.film_fwd(x, mul, add)
                ck.check("film_fwd", y.t, ref, R.bound(ref, mag, R.C_FILM), ctx)
                guards(ck, "guards", ctx, y)
            runs = []
            for _ in range(2):
                o = (Out((B, N, C), torch.float32), Out((B, C), torch.float32), Out((B, C), torch.float32))
                ops.film_bwd(to_dev(dy), to_dev(x), to_dev(mul), o[0].t, o[1].t, o[2].t)
                runs.append(o)
            r = R.film_bwd(dy, x, mul)
            for k, o in zip(("dx", "dmul", "dadd"), runs[0]):
                ck.check(f"film_bwd {k}", o.t, r[k], R.bound(r[k], r["mag_" + k], R.C_FILM), ctx)
            for a, b in zip(runs[0], runs[1]):
                ck.exact("film_bwd deterministic", b.t, a.t, ctx)
            guards(ck, "guards", ctx, *runs[0], *runs[1])
    B, N, C = 2, 4100, 512                                  # film_fwd past the 4096-block cap (a float4 per thread)
    assert B * N * C // 4 > SWEEP_DECODER
    x, mul, add = rnd(B, N, C, seed=31), rnd(B, C, seed=32), rnd(B, C, seed=33)
    y = Out((B, N, C), torch.float32)
    ops.film_fwd(to_dev(x), to_dev(mul), to_dev(add), y.t)
    ref, mag = R.film_fwd(x, mul, add)
    ck.check("film_fwd", y.t, ref, R.bound(ref, mag, R.C_FILM), "past the grid cap")
    guards(ck, "guards", "film_fwd past the grid cap", y)
    finish(ck)


# (B, C, h, w, H, W, ld).  The last two pass the 16384-block cap (an element per thread): the forward with B·C·H·W outputs,
# the backward (a downsample) with B·C·h·w inputs
UPSAMPLE = ((1, 3, 14, 14, 224, 224, 3), (2, 3, 7, 7, 20, 20, 5), (2, 2, 1, 1, 5, 5, 2), (2, 3, 3, 6, 7, 9, 3), (2, 3, 20, 9, 7, 4, 4),
            (2, 48, 14, 14, 224, 224, 48), (2, 33, 256, 256, 64, 64, 35))


def test_upsample_bilinear(ops):
    ck = R.Checker()
    assert UPSAMPLE[-2][0] * UPSAMPLE[-2][1] * 224 * 224 > SWEEP_HEADS and 2 * 33 * 256 * 256 > SWEEP_HEADS
    for B, C, h, w, H, W, ld in UPSAMPLE:                    # three downsample (H < h, W < w)
        ctx = f"B={B} C={C} {h}x{w} -> {H}x{W} ld={ld}"
        tok = rnd(B * h * w, ld, seed=h * w + H)
        dtok = torch.full((B * h * w, ld + 2), float("nan"), device=dev())
        dtok[:, :ld] = to_dev(tok)
        out = Out((B, C, H, W), torch.float32)
        ops.upsample_bilinear(dtok[:, :C] if ld == C else dtok[:, :ld], B, C, h, w, H, W, out.t)
        img = R.tokens_to_image(tok, B, C, h, w)
        ref = R.upsample(img, H, W)
        ck.check("upsample forward", out.t, ref, R.bound(ref, R.upsample_mag(img, H, W), R.C_UPSAMPLE), ctx)
        dout = rnd(B, C, H, W, seed=H * W + h)
        runs = []
        for _ in range(2):
            d = Out((B * h * w, C), torch.float32, ld=ld)
            ops.upsample_bilinear(to_dev(dout), B, C, h, w, H, W, d.t, backward=True)
            runs.append(d)
        ref_b = R.image_to_tokens(R.upsample_bwd(dout.double(), h, w))
        mag_b = R.image_to_tokens(R.upsample_mag(dout.double(), h, w, backward=True))
        ck.check("upsample backward", runs[0].t, ref_b, R.bound(ref_b, mag_b, R.C_UPSAMPLE), ctx)
        ck.exact("upsample backward deterministic", runs[1].t, runs[0].t, ctx)
        guards(ck, "guards", ctx, out, *runs)
    finish(ck)


def test_segment_mean_forward(ops):
    ck = R.Checker()
    for B, n, C, ld in ((2, 1, 5, 5), (3, 50, 1, 1), (2, 49, 300, 300), (2, 7, 300, 307), (5, 196, 64, 64)):
        ctx = f"B={B} n={n} C={C} ld={ld}"
        x = rnd(B * n, ld, seed=n + C, shift=0.5)
        outs = []
        for _ in range(2):
            o = Out((B, C), torch.float32)
            ops.segment_mean(to_dev(x)[:, :C] if ld != C else to_dev(x), B, n, o.t)
            outs.append(o)
        ref, mag = R.segment_mean(x, B, n, C)
        ck.check("segment_mean forward", outs[0].t, ref, R.bound(ref, mag, R.C_SEGMENT), ctx)
        ck.exact("segment_mean deterministic", outs[1].t, outs[0].t, ctx)
        guards(ck, "guards", ctx, *outs)
    finish(ck)


def test_colsum_adds_into_out(ops):
    ck = R.Checker()
    for dt in DT:
        for M in (1, 1023, 1025, 5000):
            for N, lda in ((70, 70), (130, 137)):
                ctx = f"{dt} M={M} N={N} lda={lda}"
                a = rnd(M, lda, seed=M + N, shift=0.25).to(dt)
                o0 = rnd(N, seed=N)
                out = Out((N,), torch.float32, init=o0)
                ops.colsum(to_dev(a)[:, :N], out.t)
                ref, mag = R.colsum(a[:, :N].double())
                ref = ref + o0.double()
                ck.check("colsum", out.t, ref, R.bound(ref, mag + o0.double().abs(), R.C_COLSUM), ctx)
                guards(ck, "guards", ctx, out)
    finish(ck)


def test_embed_bwd_accumulates(ops):
    ck = R.Checker()
    V, D = 40, 68
    for rows, pad_id in ((300, 0), (17, -1), (5000, 7), (8000, 3)):        # the last: rows·D threads past the 2048-block cap
        ctx = f"rows={rows} pad_id={pad_id}"
        g = torch.Generator().manual_seed(rows)
        ids = torch.randint(0, 6, (rows,), generator=g)                       # heavy repetition of a few ids
        ids[::7] = 3
        ids[1::11] = pad_id if pad_id >= 0 else 5
        ids[2::13] = -1
        ids[3::17] = V
        ids[4::19] = V + 1000
        dx = rnd(rows, D, seed=rows + 1)
        t0 = rnd(V, D, seed=3)
        dt_ = Out((V, D), torch.float32, init=t0)
        ops.embed_bwd(to_dev(ids), to_dev(dx), dt_.t, pad_id=pad_id)
        ref, mag = R.embed_bwd(ids, dx.double(), V, pad_id)
        ref = ref + t0.double()
        ck.check("embed_bwd", dt_.t, ref, R.bound(ref, mag + t0.double().abs(), R.C_EMBED_BWD), ctx)
        guards(ck, "guards", ctx, dt_)
    finish(ck)


def test_dicece(ops):
    ck = R.Checker()
    for B, C, H, W in ((2, 8, 1, 1), (2, 8, 15, 17), (2, 8, 17, 241), (2, 8, 5, 3277), (300, 8, 15, 17), (3, 2, 16, 16), (2, 3, 64, 65)):
        ctx = f"B={B} C={C} {H}x{W}"
        z = rnd(B, C, H, W, seed=B + C + H * W, scale=3.0)
        lab = torch.randint(0, C - 1, (B, 1, H, W), generator=torch.Generator().manual_seed(H * W)).float()    # class C-1 in no label
        runs = []
        for _ in range(2):
            o = (Out((1,), torch.float32), Out((B, C, H, W), torch.float32))
            ops.dicece_fwd_bwd(to_dev(z), to_dev(lab), out=(o[0].t, o[1].t))
            runs.append(o)
        loss, dz, mag, mag_loss = R.dicece(z.double(), lab.double())
        ck.check("dicece dlogits", runs[0][1].t, dz, R.bound(dz, mag, R.C_DICE_GRAD), ctx)
        ref_l = torch.tensor([loss], dtype=R.F64)
        ck.check("dicece loss", runs[0][0].t, ref_l, R.bound(ref_l, torch.tensor([mag_loss], dtype=R.F64), R.C_DICE_LOSS), ctx)
        ck.exact("dicece deterministic loss", runs[1][0].t, runs[0][0].t, ctx)
        ck.exact("dicece deterministic dlogits", runs[1][1].t, runs[0][1].t, ctx)
        guards(ck, "guards", ctx, *runs[0], *runs[1])
    finish(ck)


# ------------------------------------------------------------------------------------------ argument contract
def test_wrappers_refuse_bad_operands(ops, UiaError):
    """Every case below is refused before launch; every buffer is valid for the memory it describes."""
    f32 = lambda *s: torch.zeros(*s, device=dev())                           # noqa: E731
    b16 = lambda *s: torch.zeros(*s, device=dev(), dtype=torch.bfloat16)      # noqa: E731
    nc = lambda *s: f32(*s[:-1], 2 * s[-1])[..., ::2]                         # noqa: E731  non-contiguous view of valid memory
    cases = {
        "act_bwd y dtype": lambda: ops.act_bwd(b16(64), f32(64), "gelu", b16(64)),
        "act_bwd out dtype": lambda: ops.act_bwd(f32(64), f32(64), "gelu", b16(64)),
        "act_bwd y short": lambda: ops.act_bwd(f32(64), f32(63), "relu", f32(64)),
        "act_bwd out short": lambda: ops.act_bwd(f32(64), f32(64), "relu", f32(60)),
        "act_bwd non-contiguous": lambda: ops.act_bwd(f32(64), nc(64), "relu", f32(64)),
        "act_bwd int dtype": lambda: ops.act_bwd(torch.zeros(64, dtype=torch.int32, device=dev()), f32(64), "relu", f32(64)),
        "film_fwd bf16 x": lambda: ops.film_fwd(b16(2, 3, 8), f32(2, 8), f32(2, 8), f32(2, 3, 8)),
        "film_fwd mul short": lambda: ops.film_fwd(f32(2, 3, 8), f32(1, 8), f32(2, 8), f32(2, 3, 8)),
        "film_fwd y short": lambda: ops.film_fwd(f32(2, 3, 8), f32(2, 8), f32(2, 8), f32(2, 2, 8)),
        "film_fwd non-contiguous": lambda: ops.film_fwd(nc(2, 3, 8), f32(2, 8), f32(2, 8), f32(2, 3, 8)),
        "film_bwd dmul short": lambda: ops.film_bwd(f32(2, 3, 8), f32(2, 3, 8), f32(2, 8), f32(2, 3, 8), f32(8), f32(2, 8)),
        "film_bwd bf16 dy": lambda: ops.film_bwd(b16(2, 3, 8), f32(2, 3, 8), f32(2, 8), f32(2, 3, 8), f32(2, 8), f32(2, 8)),
        "im2col3x3 cols short": lambda: ops.im2col3x3(f32(2, 10, 8), f32(2 * 9, 9 * 8 - 4), 3, 3),
        "im2col3x3 bf16 x": lambda: ops.im2col3x3(b16(2, 10, 8), f32(2 * 9, 9 * 8), 3, 3),
        "im2col3x3 tok_off negative": lambda: ops.im2col3x3(f32(2, 10, 8), f32(2 * 9, 9 * 8), 3, 3, tok_off=-1),
        "im2col3x3 grid past x": lambda: ops.im2col3x3(f32(2, 10, 8), f32(2 * 9, 9 * 8), 3, 3, tok_off=2),
        "im2col3x3 non-contiguous": lambda: ops.im2col3x3(nc(2, 10, 8), f32(2 * 9, 9 * 8), 3, 3),
        "col2im3x3 dcols short": lambda: ops.col2im3x3(f32(2 * 9, 9 * 8 - 4), f32(2, 10, 8), 3, 3),
        "col2im3x3 bf16 dx": lambda: ops.col2im3x3(f32(2 * 9, 9 * 8), b16(2, 10, 8), 3, 3),
        "unshuffle tmp rows": lambda: ops.unshuffle(f32(2 * 4 * 16 - 1, 16), f32(2, 8, 8), 2, 1, 1, 4, 4),
        "unshuffle tmp narrow": lambda: ops.unshuffle(f32(2 * 16, 15), f32(2, 16, 16), 2, 1, 1, 4, 4),
        "unshuffle out short": lambda: ops.unshuffle(f32(2 * 16, 16), f32(2, 16, 15), 2, 1, 1, 4, 4),
        "unshuffle int tmp": lambda: ops.unshuffle(torch.zeros(2 * 16, 16, dtype=torch.int16, device=dev()), f32(2, 16, 16), 2, 1, 1, 4, 4),
        "shuffle strided dtmp": lambda: ops.shuffle(f32(2, 16, 16), f32(2 * 16, 20)[:, :16], 2, 1, 1, 4, 4),
        "shuffle dout short": lambda: ops.shuffle(f32(2, 16, 15), f32(2 * 16, 16), 2, 1, 1, 4, 4),
        "shuffle bf16 dout": lambda: ops.shuffle(b16(2, 16, 16), f32(2 * 16, 16), 2, 1, 1, 4, 4),
        "layernorm_bwd_affine bf16 x": lambda: ops.layernorm_bwd_affine(f32(4, 8), b16(4, 8), f32(8), 1e-5, f32(4, 8), f32(8), f32(8)),
        "layernorm_bwd_affine dx short": lambda: ops.layernorm_bwd_affine(f32(4, 8), f32(4, 8), f32(8), 1e-5, f32(3, 8), f32(8), f32(8)),
        "layernorm_bwd_affine ragged dy": lambda: ops.layernorm_bwd_affine(f32(33), f32(33), f32(8), 1e-5, f32(33), f32(8), f32(8)),
        "layernorm_bwd_affine g_beta short": lambda: ops.layernorm_bwd_affine(f32(4, 8), f32(4, 8), f32(8), 1e-5, f32(4, 8), f32(8), f32(4)),
        "layernorm_bwd_affine dres short": lambda: ops.layernorm_bwd_affine(f32(4, 8), f32(4, 8), f32(8), 1e-5, f32(4, 8), f32(8), f32(8), dres=f32(2, 8)),
        "layernorm_bwd_affine non-contiguous x": lambda: ops.layernorm_bwd_affine(f32(4, 8), nc(4, 8), f32(8), 1e-5, f32(4, 8), f32(8), f32(8)),
        "colsum out short": lambda: ops.colsum(f32(10, 8), f32(7)),
        "colsum bf16 out": lambda: ops.colsum(f32(10, 8), b16(8)),
        "upsample image shape": lambda: ops.upsample_bilinear(f32(2 * 4, 3), 2, 3, 2, 2, 5, 5, f32(2, 3, 5, 4)),
        "upsample token rows": lambda: ops.upsample_bilinear(f32(2 * 4 - 1, 3), 2, 3, 2, 2, 5, 5, f32(2, 3, 5, 5)),
        "segment_mean out short": lambda: ops.segment_mean(f32(2 * 3, 5), 2, 3, f32(1, 5)),
        "segment_mean bf16": lambda: ops.segment_mean(b16(2 * 3, 5), 2, 3, f32(2, 5)),
        "cast dst short": lambda: ops.cast(f32(64), b16(60)),
        "cast bf16 src": lambda: ops.cast(b16(64), f32(64)),
        "transpose_cast shape": lambda: ops.transpose_cast(f32(4, 8), f32(4, 8)),
        "fill_cls cls short": lambda: ops.fill_cls(f32(2, 3, 8), f32(4), None),
        "embed out short": lambda: ops.embed(torch.zeros(2, 3, dtype=torch.int64, device=dev()), f32(5, 8), f32(3, 8), None, f32(5, 8)),
        "embed int32 ids": lambda: ops.embed(torch.zeros(2, 3, dtype=torch.int32, device=dev()), f32(5, 8), f32(3, 8), None, f32(6, 8)),
        "embed_packed pos_idx short": lambda: ops.embed_packed(torch.zeros(4, dtype=torch.int64, device=dev()), torch.zeros(3, dtype=torch.int64, device=dev()),
                                                               f32(5, 8), f32(3, 8), None, f32(4, 8)),
        "embed_bwd dx short": lambda: ops.embed_bwd(torch.zeros(4, dtype=torch.int64, device=dev()), f32(3, 8), f32(5, 8)),
        "gather_rows dst short": lambda: ops.gather_rows(f32(5, 8), torch.zeros(4, dtype=torch.int64, device=dev()), f32(3, 8)),
        "dicece label short": lambda: ops.dicece_fwd_bwd(f32(2, 3, 4, 4), f32(2, 1, 4, 3)),
        "dicece dlogits short": lambda: ops.dicece_fwd_bwd(f32(2, 3, 4, 4), f32(2, 1, 4, 4), out=(f32(1), f32(2, 3, 4, 3))),
        "dicece loss bf16": lambda: ops.dicece_fwd_bwd(f32(2, 3, 4, 4), f32(2, 1, 4, 4), out=(b16(1), f32(2, 3, 4, 4))),
        # refused by the launchers (the shapes are well formed, the kernels do not take them)
        "dicece C = 1": lambda: ops.dicece_fwd_bwd(f32(2, 1, 4, 4), f32(2, 1, 4, 4)),
        "dicece C = 9 > DICE_MAXC": lambda: ops.dicece_fwd_bwd(f32(2, 9, 4, 4), f32(2, 1, 4, 4)),
        "layernorm_bwd_affine D = 1028 > 1024": lambda: ops.layernorm_bwd_affine(f32(2, 1028), f32(2, 1028), f32(1028), 1e-5, f32(2, 1028), f32(1028), f32(1028)),
        "layernorm_bwd_affine D % 4 != 0": lambda: ops.layernorm_bwd_affine(f32(2, 6), f32(2, 6), f32(6), 1e-5, f32(2, 6), f32(6), f32(6)),
        "film_fwd C % 4 != 0": lambda: ops.film_fwd(f32(3, 4, 2), f32(3, 2), f32(3, 2), f32(3, 4, 2)),
        "film_bwd 256 % C != 0": lambda: ops.film_bwd(f32(3, 4, 96), f32(3, 4, 96), f32(3, 96), f32(3, 4, 96), f32(3, 96), f32(3, 96)),
    }
    missed = []
    for name, call in cases.items():
        try:
            call()
        except UiaError:
            continue
        missed.append(name)
    torch.cuda.synchronize()
    assert not missed, f"accepted: {missed}"
