"""-m gpu: the DINOv2 UNet segmentation decoder on the HIP path.  Every kernel against float64 at ragged shapes (3x3 conv with two sources and its
data / weight gradients, BatchNorm + ReLU train / eval with the running buffers, the transposed conv, the align_corners upsample, the antialiased
bicubic resize), the whole decoder against the reference's recorded outputs (tests/golden/dino_seg_small.npz) and at full geometry against the
float64 restatement (tests/unet_reference.py), determinism of a training step, and refusals before launch.
Bars (max |error| / max |reference| per tensor): kernels 1e-4 in fp32, 1e-2 in bf16 (reference computed from the bf16-rounded operands);
the decoder end to end 1e-3 in fp32, 1e-2 in bf16."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_reference as UR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KBAR = {torch.float32: 1e-4, torch.bfloat16: 1e-2}
DBAR = {torch.float32: 1e-3, torch.bfloat16: 1e-2}
F64 = torch.float64


def rel(a, b, floor=0.0):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(float(b.abs().max()), floor, 1e-30))


def dev(t, dt):
    """(device tensor in dt, the float64 CPU value it holds)"""
    d = t.to(dt).cuda().contiguous()
    return d, d.double().cpu()


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def nchw(t):
    return t.permute(0, 3, 1, 2)


DTS = [torch.float32, torch.bfloat16]
# (B, H, W, C1, C2, N): the MFMA path (channels % 32) and the direct path, 1x1 .. 74x74 grids, unequal sources
CONV_SHAPES = [(2, 5, 5, 64, 32, 96), (1, 37, 37, 768, 0, 384), (2, 1, 1, 192, 64, 96), (1, 74, 74, 64, 64, 96), (2, 37, 37, 768, 0, 3),
               (1, 74, 74, 4, 6, 2), (3, 5, 5, 6, 0, 3), (1, 37, 37, 192, 0, 2)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3x3_forward_dgrad_wgrad(shape, dt):
    from uia_hip import functional as UF, ops
    B, H, W, C1, C2, N = shape
    g = torch.Generator().manual_seed(hash(shape) % 1000)
    x1, x1r = dev(torch.randn(B, H, W, C1, generator=g), dt)
    x2, x2r = dev(torch.randn(B, H, W, C2, generator=g), dt) if C2 else (None, None)
    w32 = torch.randn(N, C1 + C2, 3, 3, generator=g) / (9 * (C1 + C2)) ** 0.5
    bias = torch.randn(N, generator=g).cuda()
    wd = UF.conv3_rows(w32.cuda(), dt)
    wr = wd.double().cpu().reshape(N, 3, 3, C1 + C2).permute(0, 3, 1, 2)
    xr = torch.cat([x1r, x2r], dim=3) if C2 else x1r
    yr = nhwc(F.conv2d(nchw(xr), wr, bias.double().cpu(), padding=1))
    y = ops.conv_igemm(ops.CONV3, x1, x2, wd, N, bias=bias)
    assert rel(y, yr) < KBAR[dt], rel(y, yr)

    dy, dyr = dev(torch.randn(B, H, W, N, generator=g), dt)
    xin = nchw(xr).clone().requires_grad_(True)
    wq = wr.clone().requires_grad_(True)
    F.conv2d(xin, wq, padding=1).backward(nchw(dyr))
    dx_ref, dw_ref = nhwc(xin.grad), wq.grad
    wb = UF.conv3_dgrad_rows(w32.cuda(), dt)
    r = ops.conv_igemm(ops.CONV3, dy, None, wb, C1 + C2, n1=C1)
    dx = torch.cat(r, dim=3) if C2 else r
    # the data gradient's reference uses the weight as rounded to dt
    assert rel(dx, dx_ref) < KBAR[dt], rel(dx, dx_ref)
    dw = ops.conv_wgrad(ops.CONV3, x1, x2, dy, N).reshape(N, 3, 3, C1 + C2).permute(0, 3, 1, 2)
    assert rel(dw, dw_ref) < KBAR[dt], rel(dw, dw_ref)
    db = ops.colsum_ordered(dy)
    assert rel(db, dyr.sum(dim=(0, 1, 2))) < KBAR[torch.float32]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(2, 37, 37, 768, 384), (2, 5, 3, 192, 96), (1, 12, 12, 96, 3), (2, 6, 6, 64, 32)])
def test_conv_transpose_forward_backward(shape, dt):
    from uia_hip import functional as UF
    B, h, w, Cin, Cout = shape
    g = torch.Generator().manual_seed(Cin + Cout)
    x, xr = dev(torch.randn(B, h, w, Cin, generator=g), dt)
    W = (torch.randn(Cin, Cout, 2, 2, generator=g) / (4 * Cin) ** 0.5).cuda().requires_grad_(True)
    b = torch.randn(Cout, generator=g).cuda().requires_grad_(True)
    x.requires_grad_(True)
    y = UF.UnetConvTransposeFn.apply(x, W, b)
    Wr = W.detach().to(dt).double().cpu().requires_grad_(True)
    br = b.detach().double().cpu().requires_grad_(True)
    xq = nchw(xr).clone().requires_grad_(True)
    yr = F.conv_transpose2d(xq, Wr, br, stride=2)
    assert rel(y, nhwc(yr)) < KBAR[dt]
    dy, dyr = dev(torch.randn(*y.shape, generator=g), dt)
    y.backward(dy)
    yr.backward(nchw(dyr))
    assert rel(x.grad, nhwc(xq.grad)) < KBAR[dt]
    assert rel(W.grad, Wr.grad) < KBAR[dt]
    assert rel(b.grad, br.grad) < KBAR[torch.float32]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(2, 37, 37, 96), (3, 5, 7, 3), (1, 74, 74, 192), (24, 4, 4, 2)])
def test_batchnorm_relu_train_eval(shape, dt):
    from uia_hip import ops
    B, H, W, C = shape
    g = torch.Generator().manual_seed(C)
    y, yr = dev(3.0 + 2.0 * torch.randn(B, H, W, C, generator=g), dt)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).cuda()
    beta = (0.1 * torch.randn(C, generator=g)).cuda()
    rm, rv = (0.1 * torch.randn(C, generator=g)).cuda(), (1 + 0.1 * torch.rand(C, generator=g)).cuda()
    nbt = torch.zeros((), dtype=torch.int64).cuda()
    rm0, rv0 = rm.double().cpu(), rv.double().cpu()
    out, mean, invstd, scale, shift = ops.bn_fwd(y, gamma, beta, rm, rv, nbt, True, 0.1, 1e-5)
    yq = nchw(yr).clone().requires_grad_(True)
    gq, bq = gamma.double().cpu().requires_grad_(True), beta.double().cpu().requires_grad_(True)
    rmr, rvr = rm0.clone(), rv0.clone()
    outr = torch.relu(F.batch_norm(yq, rmr, rvr, gq, bq, training=True, momentum=0.1, eps=1e-5))
    assert rel(out, nhwc(outr)) < KBAR[dt]
    assert rel(rm, rmr) < 1e-5 and rel(rv, rvr) < 1e-5 and int(nbt) == 1
    dout, doutr = dev(torch.randn(B, H, W, C, generator=g), dt)
    dy, dgamma, dbeta = ops.bn_relu_bwd(y, dout, scale, shift, mean, invstd, gamma)
    outr.backward(nchw(doutr))
    assert rel(dy, nhwc(yq.grad)) < KBAR[dt]
    assert rel(dgamma, gq.grad) < KBAR[dt] and rel(dbeta, bq.grad) < KBAR[dt]
    # eval: the running statistics, buffers untouched
    rm1, rv1 = rm.clone(), rv.clone()
    ev = ops.bn_fwd(y, gamma, beta, rm, rv, nbt, False, 0.1, 1e-5)[0]
    evr = torch.relu(F.batch_norm(nchw(yr), rm1.double().cpu(), rv1.double().cpu(), gamma.double().cpu(), beta.double().cpu(), training=False, eps=1e-5))
    assert rel(ev, nhwc(evr)) < KBAR[dt]
    assert torch.equal(rm, rm1) and torch.equal(rv, rv1) and int(nbt) == 1


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("f", [2, 4, 8, 16])
def test_upsample_align_corners(f, dt):
    from uia_hip import functional as UF
    B, H, W, C = 2, 37 if f < 16 else 7, 5, 3 if f == 16 else 96
    g = torch.Generator().manual_seed(f)
    x, xr = dev(torch.randn(B, H, W, C, generator=g), dt)
    x.requires_grad_(True)
    y = UF.UpsampleACFn.apply(x, f)
    xq = nchw(xr).clone().requires_grad_(True)
    yr = F.interpolate(xq, scale_factor=float(f), mode="bilinear", align_corners=True)
    assert rel(y, nhwc(yr)) < KBAR[dt]
    dy, dyr = dev(torch.randn(*y.shape, generator=g), dt)
    y.backward(dy)
    yr.backward(nchw(dyr))
    assert rel(x.grad, nhwc(xq.grad)) < KBAR[dt]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("sizes", [(592, 518, 1, 2), (96, 84, 2, 3), (40, 40, 2, 3), (37, 50, 1, 2)])
def test_resize_bicubic_antialias(sizes, dt):
    from uia_hip import functional as UF
    Hi, Ho, B, C = sizes
    g = torch.Generator().manual_seed(Hi)
    x, xr = dev(torch.randn(B, Hi, Hi, C, generator=g), dt)
    x.requires_grad_(True)
    y = UF.ResizeAAFn.apply(x, (Ho, Ho))
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, C, Ho, Ho)
    xq = nchw(xr).clone().requires_grad_(True)
    yr = UR.resize(xq, (Ho, Ho))
    assert rel(y, yr) < KBAR[torch.float32]
    dy = torch.randn(B, C, Ho, Ho, generator=g)
    y.backward(dy.cuda())
    yr.backward(dy.double())
    assert rel(x.grad, nhwc(xq.grad)) < KBAR[dt]


def build_decoder(S, P, dt):
    from src.third_party.dino.dinov2 import UNetDecoder
    from uia_hip import functional as UF
    UF.set_compute_dtype(dt)
    dec = UNetDecoder(S["embed_dim"], S["num_classes"], image_size=S["image_size"], resize_image=True, patch_size=S["patch_size"])
    dec.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in P.items()})
    return dec.cuda()


def check_decoder(S, P, maps, dlogits, ref, dt, bar, grad_bars=None):
    """ref: train_out, buf:*, grad:*, eval_out (numpy or tensors).  grad_bars: per-parameter bars replacing `bar` for the gradients (a parameter
    missing from it is not compared)."""
    from uia_hip import functional as UF
    try:
        dec = build_decoder(S, P, dt)
        dec.train()
        out = dec([m.float().cuda() for m in maps])
        (out * dlogits.float().cuda()).sum().backward()
        t = lambda v: torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v   # noqa: E731
        assert rel(out, t(ref["train_out"])) < bar, rel(out, t(ref["train_out"]))
        sd = dict(dec.state_dict())
        for k, v in sd.items():
            if "num_batches" in k:
                assert int(v) == 1, k
            elif "running" in k:
                assert rel(v, t(ref["buf:" + k])) < bar, (k, rel(v, t(ref["buf:" + k])))
        gscale = {}
        for k, p in dec.named_parameters():
            blk = k.split(".")[0] + "." + k.split(".")[1]
            gscale[blk] = max(gscale.get(blk, 0.0), float(t(ref["grad:" + k]).abs().max()))
        errs = {}
        for k, p in dec.named_parameters():
            blk = k.split(".")[0] + "." + k.split(".")[1]
            # the biases of convs before train-mode BN have a zero gradient: measured against their block's largest gradient
            floor = gscale[blk] if k.endswith(".0.bias") and ("conv.0" in k) else 0.0
            if grad_bars is None or k in grad_bars:
                errs[k] = (rel(p.grad, t(ref["grad:" + k]), floor), bar if grad_bars is None else grad_bars[k])
        assert all(e < b for e, b in errs.values()), " ".join(f"{k}={e:.1e}/{b:.1e}" for k, (e, b) in errs.items())
        dec.eval()
        with torch.no_grad():
            ev = dec([m.float().cuda() for m in maps])
        assert rel(ev, t(ref["eval_out"])) < bar, rel(ev, t(ref["eval_out"]))
    finally:
        UF.set_compute_dtype(torch.bfloat16)


def test_decoder_matches_reference_golden_fp32():
    S = UR.SMALL
    g = np.load(os.path.join(HERE, "golden", "dino_seg_small.npz"))
    P = UR.seeded_state(S["embed_dim"], S["num_classes"], S["seed"])
    maps, dlogits = UR.seeded_inputs(**S)
    check_decoder(S, P, maps, dlogits, dict(g), torch.float32, DBAR[torch.float32])


_FULL = {}


def full_reference():
    """The decoder at full geometry (B = 2, 518 px, 768 -> 2 classes) in float64, and the same restatement run in float32 on the CPU: the
    latter measures how far plain fp32 arithmetic can land from float64 on this problem."""
    if not _FULL:
        S = dict(embed_dim=768, image_size=518, patch_size=14, num_classes=2, batch=2, seed=77)
        P = UR.seeded_state(S["embed_dim"], S["num_classes"], S["seed"])
        maps, dlogits = UR.seeded_inputs(**S)
        names = [k for k, _ in UR.state_shapes(768, 2) if "running" not in k and "num_batches" not in k]
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        grads = {}
        for dt in (F64, torch.float32):
            Pg = {k: (v.to(dt).clone().requires_grad_(True) if k in names else (v.to(dt) if v.is_floating_point() else v.clone())) for k, v in P.items()}
            out, bufs = UR.decoder_forward(Pg, [m.to(dt) for m in maps], S["image_size"], S["patch_size"], training=True)
            (out * dlogits.to(dt)).sum().backward()
            grads[dt] = {k: Pg[k].grad.double() for k in names}
            if dt == F64:
                ref = {"train_out": out.detach()}
                ref.update({"buf:" + k: v for k, v in bufs.items()})
                ref.update({"grad:" + k: grads[dt][k] for k in names})
                with torch.no_grad():
                    ref["eval_out"] = UR.decoder_forward(P, maps, S["image_size"], S["patch_size"], training=False, bufs=bufs)[0]
        fp32_err = {k: float((grads[torch.float32][k] - grads[F64][k]).abs().max() / grads[F64][k].abs().max()) for k in names}
        _FULL.update(S=S, P=P, maps=maps, dlogits=dlogits, ref=ref, fp32_err=fp32_err, names=names)
    return _FULL


def test_decoder_full_geometry_fp32():
    """Forward, eval output and buffers at 1e-3.  Gradients: the deep blocks' weight gradients are ill-conditioned on this problem (train-mode
    BatchNorm after ReLU masks; PyTorch's own fp32 run of the restatement lands 1e-2 from float64 on up1.conv.0.weight), so each gradient's bar
    is max(1e-3, 3x the error of that fp32 run); the zero-gradient conv biases before BatchNorm are measured against their block at 1e-3."""
    R = full_reference()
    bars = {k: DBAR[torch.float32] if (k.endswith(".0.bias") and "conv.0" in k) else max(DBAR[torch.float32], 3.0 * e) for k, e in R["fp32_err"].items()}
    check_decoder(R["S"], R["P"], R["maps"], R["dlogits"], R["ref"], torch.float32, DBAR[torch.float32], grad_bars=bars)


def test_decoder_full_geometry_bf16():
    """Forward, eval output and BatchNorm buffers at 1e-2.  The gradients are not compared at this geometry in bf16: each BatchNorm backward sums
    dz·x̂ over up to 700k pixels of bf16-rounded gradients whose exact sum nearly cancels, so the parameter gradients land 1e-2 .. 2.5e-1 from float64
    even at the last block.  They are covered in fp32 here and per kernel in bf16 above."""
    R = full_reference()
    check_decoder(R["S"], R["P"], R["maps"], R["dlogits"], R["ref"], torch.bfloat16, DBAR[torch.bfloat16], grad_bars={})


def test_training_step_is_deterministic():
    from uia_hip import functional as UF
    S = dict(embed_dim=256, image_size=112, patch_size=14, num_classes=2, batch=3, seed=5)
    P = UR.seeded_state(S["embed_dim"], S["num_classes"], S["seed"])
    maps, dlogits = UR.seeded_inputs(**S)
    results = []
    for _ in range(2):
        dec = build_decoder(S, P, torch.bfloat16)
        dec.train()
        out = dec([m.float().cuda() for m in maps])
        loss = (out * dlogits.float().cuda()).sum()
        loss.backward()
        results.append((loss.detach().clone(), {k: v.clone() for k, v in dec.state_dict().items()}, {k: p.grad.clone() for k, p in dec.named_parameters()}))
    UF.set_compute_dtype(torch.bfloat16)
    (l0, s0, g0), (l1, s1, g1) = results
    assert torch.equal(l0, l1)
    assert all(torch.equal(s0[k], s1[k]) for k in s0)
    assert all(torch.equal(g0[k], g1[k]) for k in g0)


def test_refusals_before_launch():
    from uia_hip import ops
    from uia_hip._lib import UiaError
    x = torch.zeros(1, 4, 4, 32, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(16, 9 * 32, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(UiaError, match="w must be contiguous"):
        ops.conv_igemm(ops.CONV3, x, None, w[:, :100], 16)
    with pytest.raises(UiaError, match="dtype"):
        ops.conv_igemm(ops.CONV3, x, x.float(), w, 16)
    with pytest.raises(UiaError, match="NHWC"):
        ops.conv_igemm(ops.CONV3, x.permute(0, 3, 1, 2), None, w, 16)
    with pytest.raises(UiaError, match="split N1"):
        ops.conv_igemm(ops.CONV3, x, None, w, 16, n1=17)
    with pytest.raises(UiaError, match="even"):
        ops.conv_igemm(ops.CONVT_BWD, torch.zeros(1, 5, 4, 32, device="cuda", dtype=torch.bfloat16), None, torch.zeros(8, 128, device="cuda", dtype=torch.bfloat16), 8)
    with pytest.raises(UiaError, match="beyond 3x"):
        ops.resize_aa(torch.zeros(1, 40, 40, 2, device="cuda"), (10, 10))
    with pytest.raises(UiaError, match="not a multiple"):
        ops.upsample_ac(torch.zeros(1, 10, 10, 2, device="cuda"), 4, backward=True)
    with pytest.raises(UiaError, match="fp32"):
        ops.bn_fwd(x, torch.zeros(31, device="cuda"), torch.zeros(32, device="cuda"), None, None, None, True)
    torch.cuda.synchronize()


def test_dicece_descends_on_learnable_masks():
    """Decoder training on fixed maps whose masks are a function of them: DiceCE falls within 60 steps (min of the last four < 0.8 x the first)."""
    from src.losses.dice import DiceCELoss
    from uia_hip import functional as UF
    from uia_hip.engine import FlatAdapterOptimizer, segmentation_step
    S = UR.SMALL
    P = UR.seeded_state(S["embed_dim"], S["num_classes"], S["seed"])
    maps, _ = UR.seeded_inputs(**S)
    h = S["image_size"] // S["patch_size"]
    sign = maps[-1][..., 0].reshape(-1, 1, h, h)
    labels = (torch.nn.functional.interpolate(sign.float(), size=(S["image_size"],) * 2, mode="nearest") > 0).long().cuda()
    dec = build_decoder(S, P, torch.float32)
    dec.train()
    opt = FlatAdapterOptimizer(list(dec.named_parameters()), lr=1e-2, betas=(0.9, 0.95), weight_decay=0.01, max_norm=0.0)
    crit = DiceCELoss(smooth_nr=1e-8, smooth_dr=1e-8)
    feats = [m.float().cuda() for m in maps]

    class Wrap(torch.nn.Module):
        def forward(self, x):
            return dec(x)
    losses = [float(segmentation_step(Wrap(), crit, opt, feats, labels)[0]) for _ in range(60)]
    UF.set_compute_dtype(torch.bfloat16)
    assert all(np.isfinite(losses)) and min(losses[-4:]) < 0.8 * losses[0], losses


@pytest.mark.parametrize("dtype, epochs", [("bf16", 2), ("fp32", 1)])
def test_entry_point_end_to_end(tmp_path, dtype, epochs):
    import csv
    import glob
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "nextgen-uia_amd"), root]))
    base = [sys.executable, "-m", "src.models.dino.segmentation", "--synthetic", "--synthetic_train", "8", "--synthetic_val", "4", "--synthetic_test", "4",
            "--batch_size", "4", "--num_workers", "0", "--dtype", dtype]
    r = subprocess.run(base + ["--epochs", str(epochs), "--val_every", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    best = tmp_path / "runs" / "dino_seg" / "LN-INT" / "train" / "best_model.pth"
    assert best.exists()
    state = torch.load(best, map_location="cpu")
    assert any(k.endswith("conv.1.running_var") for k in state) and all(k.startswith("decoders_dict.unet:lr=0_0001000000.") for k in state)
    r = subprocess.run(base + ["--test"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    found = glob.glob(str(tmp_path / "runs" / "dino_seg" / "LN-INT" / "test" / "**" / "results.csv"), recursive=True)
    assert found
    rows = {r[0]: r[1:] for r in csv.reader(open(found[0]))}
    for key in ("Dice", "IoU", "HD95", "ASD"):
        assert key in rows and rows[key][0] != "" and np.isfinite(float(rows[key][0])), rows
