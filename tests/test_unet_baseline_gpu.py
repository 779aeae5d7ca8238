"""-m gpu: the from-scratch UNet baseline on the HIP path, end to end.  The whole model against the reference's recorded outputs
(tests/golden/unet_baseline_small.npz, c = 8, 32x32, masks passed) and, at c = 16, B = 3, 48x48, against the float64 restatement of
tests/unet_baseline_reference.py; a one-channel batch against its three-channel repeat; determinism of a training step; descent; the entry point;
refusals before launch.  The kernels themselves are judged element by element in tests/test_unet_baseline_contract_gpu.py.

Bars (max |error| / max |reference| per tensor).  fp32: logits, buffers and eval logits 1e-3; each gradient max(1e-3, 3 x the error of the
restatement run in fp32 on the CPU against float64) — train-mode BatchNorm after sign masks and pool routing is ill-conditioned, the rule of
tests/test_dino_seg_gpu.py; the conv biases in front of a BatchNorm have an exactly zero gradient and are measured against their block's largest
gradient at 1e-3.  bf16: logits and buffers only, at max(1e-2, 2 x e_ref) with e_ref the error of the restatement run in torch.bfloat16 on the
CPU (BatchNorm statistics in fp32, as PyTorch's batch_norm keeps them) against float64 on the same inputs.  The test prints it: 4.5e-2 on the
train logits and 1.0e-2 on the eval logits at c = 16, B = 3, 48x48 with these seeds, so a flat 1e-2 would fail on arithmetic alone; the factor 2
is for rounding sites and summation orders that differ from PyTorch's.  Gradients are not compared in bf16 at model level."""
import json
import os

import numpy as np
import pytest
import torch

import unet_baseline_reference as UB

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
F64 = torch.float64
BAR32 = 1e-3
BAR16 = 1e-2


def rel(a, b, floor=0.0):
    a, b = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().double().cpu(), torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(float(b.abs().max()), floor, 1e-30))


def build_net(S, P, dt):
    from src.third_party.unet import UNet
    from uia_hip import functional as UF
    UF.set_compute_dtype(dt)
    net = UNet(S["in_channels"], S["num_classes"], init_channels=S["init_channels"])
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in P.items()})
    return net.cuda()


def device_masks(masks):
    return [m.permute(0, 2, 3, 1).to(torch.uint8).contiguous().cuda() for m in masks]


def is_zero_grad_bias(k):
    """The bias of a conv in front of a train-mode BatchNorm."""
    return ".conv_conv." in k and (k.endswith(".0.bias") or k.endswith(".4.bias"))


def block_of(k):
    return k.split(".conv_conv.")[0] if ".conv_conv." in k else k.rsplit(".", 1)[0]


def run_net(S, P, x, masks, dlogits, dt):
    """One train-mode forward / backward with the masks, then the eval forward: (train logits, state dict, gradients, eval logits)."""
    from uia_hip import functional as UF
    try:
        net = build_net(S, P, dt)
        net.train()
        out = net(x.float().cuda(), device_masks(masks))
        (out * dlogits.float().cuda()).sum().backward()
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
        state = {k: v.detach().clone() for k, v in net.state_dict().items()}
        net.eval()
        with torch.no_grad():
            ev = net(x.float().cuda())
        assert out.dtype == torch.float32 and tuple(out.shape) == (x.shape[0], S["num_classes"], x.shape[2], x.shape[3]) and out.is_contiguous()
        return out.detach(), state, grads, ev
    finally:
        UF.set_compute_dtype(torch.bfloat16)


def check_fp32(S, P, x, masks, dlogits, ref, fp32_err):
    """ref: train_out, buf:*, grad:*, eval_out.  fp32_err: per parameter, the error of the fp32 CPU restatement against float64."""
    out, state, grads, ev = run_net(S, P, x, masks, dlogits, torch.float32)
    e = rel(out, ref["train_out"])
    print(f"train logits {e:.2e}")
    assert e < BAR32, e
    for k, v in state.items():
        if "num_batches" in k:
            assert int(v) == 1, k
        elif "running" in k:
            assert rel(v, ref["buf:" + k]) < BAR32, (k, rel(v, ref["buf:" + k]))
    gscale = {}
    for k in grads:
        gscale[block_of(k)] = max(gscale.get(block_of(k), 0.0), float(torch.as_tensor(np.asarray(ref["grad:" + k])).abs().max()))
    errs = {}
    for k, gv in grads.items():
        if is_zero_grad_bias(k):
            errs[k] = (rel(gv, ref["grad:" + k], gscale[block_of(k)]), BAR32)
        else:
            errs[k] = (rel(gv, ref["grad:" + k]), max(BAR32, 3.0 * fp32_err[k]))
    worst = max(errs.items(), key=lambda kv: kv[1][0] / kv[1][1])
    print(f"worst gradient: {worst[0]} {worst[1][0]:.1e} against {worst[1][1]:.1e}")
    assert all(e < b for e, b in errs.values()), " ".join(f"{k}={e:.1e}/{b:.1e}" for k, (e, b) in errs.items() if not e < b)
    e = rel(ev, ref["eval_out"])
    print(f"eval logits {e:.2e}")
    assert e < BAR32, e


_CASES = {}


def case(name):
    """The seeded problem `name` with its float64 restatement, and the fp32 / bf16 CPU runs of the same restatement (computed once)."""
    if name not in _CASES:
        S = UB.SMALL if name == "small" else dict(in_channels=3, num_classes=2, init_channels=16, batch=3, size=48, seed=2468)
        P = UB.seeded_state(S["in_channels"], S["num_classes"], S["init_channels"], S["seed"])
        x, dlogits = UB.seeded_inputs(**S)
        masks = UB.seeded_masks(**S)
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        runs = {dt: UB.run_restatement(P, x, masks, dlogits, dt) for dt in ((F64, torch.float32) if name == "small" else (F64, torch.float32, torch.bfloat16))}
        out, bufs, grads, ev = runs[F64]
        ref = {"train_out": out, "eval_out": ev}
        ref.update({"buf:" + k: v for k, v in bufs.items()})
        ref.update({"grad:" + k: v for k, v in grads.items()})
        fp32_err = {k: float((runs[torch.float32][2][k] - v).abs().max() / max(float(v.abs().max()), 1e-30)) for k, v in grads.items()}
        _CASES[name] = dict(S=S, P=P, x=x, dlogits=dlogits, masks=masks, ref=ref, fp32_err=fp32_err, runs=runs)
    return _CASES[name]


def test_matches_reference_golden_fp32():
    R = case("small")
    g = dict(np.load(os.path.join(GOLDEN, "unet_baseline_small.npz")))
    g.update(np.load(os.path.join(GOLDEN, "unet_baseline_small_down4.npz")))
    check_fp32(R["S"], R["P"], R["x"], R["masks"], R["dlogits"], g, R["fp32_err"])


def test_c16_48px_fp32_against_restatement():
    R = case("c16")
    check_fp32(R["S"], R["P"], R["x"], R["masks"], R["dlogits"], R["ref"], R["fp32_err"])


def test_c16_48px_bf16_logits_and_buffers():
    R = case("c16")
    out, state, _, ev = run_net(R["S"], R["P"], R["x"], R["masks"], R["dlogits"], torch.bfloat16)
    cpu_out, cpu_bufs, _, cpu_ev = R["runs"][torch.bfloat16]
    ref = R["ref"]
    rows = [("train logits", out, ref["train_out"], cpu_out), ("eval logits", ev, ref["eval_out"], cpu_ev)]
    rows += [(k, v, ref["buf:" + k], cpu_bufs[k]) for k, v in state.items() if "running" in k]
    bad = []
    worst = [0.0, 0.0]
    for name, got, want, cpu in rows:
        e_ref, e = rel(cpu, want), rel(got, want)
        worst = [max(worst[0], e_ref), max(worst[1], e)]
        if name.endswith("logits") or not e < 0.5 * max(BAR16, 2.0 * e_ref):
            print(f"{name}: e_ref (bf16 restatement on the CPU) {e_ref:.2e}, HIP {e:.2e}, bar {max(BAR16, 2 * e_ref):.2e}")
        if not e < max(BAR16, 2.0 * e_ref):
            bad.append(f"{name}: HIP {e:.2e}, e_ref {e_ref:.2e}")
    print(f"worst over logits and buffers: e_ref {worst[0]:.2e}, HIP {worst[1]:.2e}")
    assert not bad, bad
    assert all(int(v) == 1 for k, v in state.items() if "num_batches" in k)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_one_channel_batch_equals_its_three_channel_repeat(dt):
    from uia_hip import functional as UF
    R = case("small")
    x1 = R["x"][:, :1].float().cuda()
    masks = device_masks(R["masks"])
    try:
        res = []
        for xin in (x1, x1.repeat(1, 3, 1, 1)):
            net = build_net(R["S"], R["P"], dt)
            net.train()
            out = net(xin, masks)
            (out * R["dlogits"].float().cuda()).sum().backward()
            res.append((out.detach(), net.encoder.in_conv.conv_conv[0].weight.grad.clone()))
    finally:
        UF.set_compute_dtype(torch.bfloat16)
    assert torch.equal(res[0][0], res[1][0])
    gw = res[0][1]
    assert torch.equal(gw, res[1][1]) and float(gw.abs().max()) > 0
    assert torch.equal(gw[:, 0], gw[:, 1]) and torch.equal(gw[:, 0], gw[:, 2])        # the gradient reaches all three slices


def test_training_step_is_deterministic():
    from src.losses.dice import DiceCELoss
    from uia_hip import functional as UF
    R = case("c16")
    labels = (R["x"][:, :1] > 0).long().cuda()
    crit = DiceCELoss(smooth_nr=1e-8, smooth_dr=1e-8)
    results = []
    try:
        for _ in range(2):
            net = build_net(R["S"], R["P"], torch.bfloat16)
            net.train()
            UF.set_dropout_seed(4242)
            loss = crit(net(R["x"].float().cuda()), labels)
            loss.backward()
            results.append((loss.detach().clone(), {k: v.clone() for k, v in net.state_dict().items()}, {k: p.grad.clone() for k, p in net.named_parameters()}))
    finally:
        UF.set_compute_dtype(torch.bfloat16)
    (l0, s0, g0), (l1, s1, g1) = results
    assert torch.isfinite(l0) and torch.equal(l0, l1)
    assert all(torch.equal(s0[k], s1[k]) for k in s0)
    assert all(torch.equal(g0[k], g1[k]) for k in g0) and all(bool(torch.isfinite(v).all()) for v in g0.values())


def test_dicece_descends_with_dropout_on():
    """c = 8, four 32x32 images, labels avg_pool5(x) > 0.5, FlatAdapterOptimizer at lr 1e-2, train mode with the generated dropout masks:
    min(last four of 60 losses) < 0.5 x the first (the reference reaches 0.03 x on this problem on the CPU)."""
    import torch.nn.functional as F
    from src.losses.dice import DiceCELoss
    from src.third_party.unet import UNet
    from uia_hip import functional as UF
    from uia_hip.engine import FlatAdapterOptimizer, segmentation_step
    g = torch.Generator().manual_seed(1)
    x = torch.rand(4, 3, 32, 32, generator=g)
    labels = (F.avg_pool2d(x.mean(1, keepdim=True), 5, stride=1, padding=2) > 0.5).long().cuda()
    assert 0.2 < float(labels.float().mean()) < 0.8
    try:
        UF.set_compute_dtype(torch.float32)
        UF.set_dropout_seed(1)
        torch.manual_seed(1)
        net = UNet(3, 2, init_channels=8).cuda()
        net.train()
        opt = FlatAdapterOptimizer(list(net.named_parameters()), lr=1e-2, betas=(0.9, 0.95), weight_decay=0.01, max_norm=0.0)
        crit = DiceCELoss(smooth_nr=1e-8, smooth_dr=1e-8)
        xd = x.cuda()
        losses = [float(segmentation_step(net, crit, opt, xd, labels)[0]) for _ in range(60)]
    finally:
        UF.set_compute_dtype(torch.bfloat16)
    print("first", losses[0], "last four", losses[-4:])
    assert all(np.isfinite(losses)) and min(losses[-4:]) < 0.5 * losses[0], losses


@pytest.mark.parametrize("dtype, epochs", [("bf16", 2), ("fp32", 1)])
def test_entry_point_end_to_end(tmp_path, dtype, epochs):
    import csv
    import glob
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "nextgen-uia_amd"), root]))
    base = [sys.executable, "-m", "src.models.baselines.segmentation", "--synthetic", "--synthetic_train", "8", "--synthetic_val", "4", "--synthetic_test", "4",
            "--img_size", "64", "--batch_size", "4", "--num_workers", "0", "--dtype", dtype]
    r = subprocess.run(base + ["--epochs", str(epochs), "--val_every", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    best = tmp_path / "runs" / "unet_seg" / "LN-INT" / "train" / "best_model.pth"
    assert best.exists()
    state = torch.load(best, map_location="cpu")
    ref = json.load(open(os.path.join(GOLDEN, "unet_baseline_keys.json")))["state"]
    assert [[k, list(v.shape)] for k, v in state.items()] == ref
    assert all(int(v) == 2 * epochs for k, v in state.items() if k.endswith("num_batches_tracked"))
    r = subprocess.run(base + ["--test"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    found = glob.glob(str(tmp_path / "runs" / "unet_seg" / "LN-INT" / "test" / "**" / "results.csv"), recursive=True)
    assert found
    rows = {r[0]: r[1:] for r in csv.reader(open(found[0]))}
    for key in ("Dice", "IoU", "HD95", "ASD"):
        assert key in rows and rows[key][0] != "" and np.isfinite(float(rows[key][0])), rows


def test_refusals_before_launch():
    from src.third_party.unet import UNet
    from uia_hip import functional as UF, ops
    from uia_hip._lib import UiaError
    net = UNet(3, 2, init_channels=8).cuda()
    with pytest.raises(ValueError, match="multiple of 16"):
        net(torch.zeros(1, 3, 40, 40, device="cuda"))
    masks = [torch.ones(1, 32 >> i, 32 >> i, 8 << i, dtype=torch.uint8, device="cuda") for i in range(5)]
    masks[1] = masks[1][:, :, :, :8].contiguous()
    with pytest.raises(ValueError, match=r"keep_masks\[1\]"):
        net(torch.zeros(1, 3, 32, 32, device="cuda"), masks)
    x = torch.zeros(1, 4, 4, 8, device="cuda", dtype=torch.bfloat16)
    blk = net.encoder.in_conv.conv_conv
    w = torch.zeros(8, 8, 3, 3, device="cuda")
    args = (w, blk[0].bias, blk[1].weight, blk[1].bias, blk[1].running_mean, blk[1].running_var, blk[1].num_batches_tracked, True, 0.1, 1e-5, 0.01)
    before = blk[1].running_mean.clone()
    for pd in (1.0, 1.5):
        with pytest.raises(UiaError, match="drop_p"):
            UF.UnetConvBNActFn.apply(x, None, *args, pd, None)
    with pytest.raises(UiaError, match="keep_mask"):
        UF.UnetConvBNActFn.apply(x, None, *args, 0.5, torch.ones(1, 4, 4, 7, dtype=torch.uint8, device="cuda"))
    with pytest.raises(UiaError, match="not 1x1 or 3x3"):
        UF.UnetConvFn.apply(x, torch.zeros(8, 8, 2, 2, device="cuda"), blk[0].bias)
    with pytest.raises(UiaError, match="unknown mode"):
        ops.conv_igemm(4, x, None, torch.zeros(8, 8, device="cuda", dtype=torch.bfloat16), 8)
    torch.cuda.synchronize()
    assert torch.equal(blk[1].running_mean, before) and int(blk[1].num_batches_tracked) == 0
