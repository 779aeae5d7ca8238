"""-m gpu: the ResNet classification baseline on the HIP path, end to end.  ResNet-18, B = 3, 64x64, two classes, against the float64
restatement of tests/resnet_reference.py: train-mode and eval-mode logits, every parameter gradient, the BatchNorm buffers after one step;
a one-channel batch; determinism; a torchvision-named state dict through --ckpt_path and the checkpoint hooks; descent; the entry point.
The kernels themselves are judged element by element in tests/test_resnet_contract_gpu.py.

Bars (max |error| / max |reference| per tensor).  fp32: 1e-3, the project's parity bound, on the logits, every gradient and every buffer.
bf16: max(1e-2, 2 x e_ref) per tensor, e_ref the error of the same restatement run in torch.bfloat16 on the CPU (BatchNorm statistics in
fp32) against float64: computed here, never taken from the HIP path.  Each test prints its figures before it asserts."""
import os

import numpy as np
import pytest
import torch

import resnet_reference as RR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = torch.float64
BAR32 = 1e-3
BAR16 = 1e-2
CASE = dict(batch=3, size=64, num_classes=2, seed=1357)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def build_net(P, dt):
    from src.third_party.resnet import resnet18
    from uia_hip import functional as UF
    UF.set_compute_dtype(dt)
    net = resnet18(num_classes=CASE["num_classes"])
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in P.items()})
    return net.cuda()


def run_net(P, x, dlogits, dt):
    """One train-mode forward / backward, then the eval forward: (train logits, state dict, gradients, eval logits)."""
    from uia_hip import functional as UF
    try:
        net = build_net(P, dt)
        net.train()
        out = net(x.float().cuda())
        (out * dlogits.float().cuda()).sum().backward()
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
        state = {k: v.detach().clone() for k, v in net.state_dict().items()}
        net.eval()
        with torch.no_grad():
            ev = net(x.float().cuda())
        assert out.dtype == torch.float32 and tuple(out.shape) == (x.shape[0], CASE["num_classes"]) and out.is_contiguous()
        return out.detach(), state, grads, ev
    finally:
        UF.set_compute_dtype(torch.bfloat16)


_CASE = {}


def case():
    """The seeded problem with its float64 restatement and the bf16 CPU run of the same restatement (computed once, left unchanged)."""
    if not _CASE:
        P = RR.seeded_state("resnet18", CASE["num_classes"], CASE["seed"])
        x, dlogits = RR.seeded_inputs(**CASE)
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _CASE.update(P=P, x=x, dlogits=dlogits, runs={dt: RR.run_restatement(P, x, dlogits, dt) for dt in (F64, torch.bfloat16)})
    return _CASE


def rows_of(run):
    out, bufs, grads, ev = run
    rows = {"train logits": out, "eval logits": ev}
    rows.update({"grad " + k: v for k, v in grads.items()})
    rows.update({"buffer " + k: v for k, v in bufs.items() if v.dtype != torch.int64})
    return rows


def got_rows(out, state, grads, ev):
    rows = {"train logits": out, "eval logits": ev}
    rows.update({"grad " + k: v for k, v in grads.items()})
    rows.update({"buffer " + k: v for k, v in state.items() if "running" in k})
    return rows


def test_fp32_logits_gradients_and_buffers_against_float64():
    R = case()
    out, state, grads, ev = run_net(R["P"], R["x"], R["dlogits"], torch.float32)
    want, got = rows_of(R["runs"][F64]), got_rows(out, state, grads, ev)
    assert set(want) == set(got) and len(grads) == 62
    errs = {k: rel(got[k], want[k]) for k in want}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"train logits {errs['train logits']:.2e}, eval logits {errs['eval logits']:.2e}, worst tensor: {worst[0]} {worst[1]:.2e}")
    print("worst gradient:", max(((k, e) for k, e in errs.items() if k.startswith("grad ")), key=lambda kv: kv[1]))
    assert all(int(v) == 1 for k, v in state.items() if "num_batches" in k)
    bad = {k: f"{e:.2e}" for k, e in errs.items() if not e < BAR32}
    assert not bad, bad


def test_bf16_logits_gradients_and_buffers_against_float64():
    R = case()
    out, state, grads, ev = run_net(R["P"], R["x"], R["dlogits"], torch.bfloat16)
    want, cpu, got = rows_of(R["runs"][F64]), rows_of(R["runs"][torch.bfloat16]), got_rows(out, state, grads, ev)
    bad, worst = [], (0.0, 0.0, "")
    for k in want:
        e_ref, e = rel(cpu[k], want[k]), rel(got[k], want[k])
        bar_ = max(BAR16, 2.0 * e_ref)
        if e / bar_ > worst[0]:
            worst = (e / bar_, e, f"{k}: HIP {e:.2e}, e_ref {e_ref:.2e}, bar {bar_:.2e}")
        if k.endswith("logits"):
            print(f"{k}: e_ref (bf16 restatement on the CPU) {e_ref:.2e}, HIP {e:.2e}, bar {bar_:.2e}")
        if not e < bar_:
            bad.append(f"{k}: HIP {e:.2e}, e_ref {e_ref:.2e}")
    print("closest to its bar:", worst[2])
    assert not bad, bad
    assert all(int(v) == 1 for k, v in state.items() if "num_batches" in k)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_one_channel_batch_equals_its_three_channel_repeat(dt):
    from uia_hip import functional as UF
    R = case()
    x1 = R["x"][:, :1].float().cuda()
    try:
        res = []
        for xin in (x1, x1.repeat(1, 3, 1, 1)):
            net = build_net(R["P"], dt)
            net.train()
            out = net(xin)
            (out * R["dlogits"].float().cuda()).sum().backward()
            res.append((out.detach(), net.conv1.weight.grad.clone()))
    finally:
        UF.set_compute_dtype(torch.bfloat16)
    assert torch.equal(res[0][0], res[1][0])
    gw = res[0][1]
    assert tuple(gw.shape) == (64, 3, 7, 7) and torch.equal(gw, res[1][1]) and float(gw.abs().max()) > 0
    assert torch.equal(gw[:, 0], gw[:, 1]) and torch.equal(gw[:, 0], gw[:, 2])        # the gradient reaches all three slices


def test_training_step_is_deterministic():
    from src.losses.focal import FocalLoss
    from uia_hip import functional as UF
    R = case()
    labels = torch.tensor([0, 1, 1]).cuda()
    crit = FocalLoss(to_onehot_y=True)
    results = []
    try:
        for _ in range(2):
            net = build_net(R["P"], torch.bfloat16)
            net.train()
            loss = crit(net(R["x"].float().cuda()), labels)
            loss.backward()
            results.append((loss.detach().clone(), {k: v.clone() for k, v in net.state_dict().items()}, {k: p.grad.clone() for k, p in net.named_parameters()}))
    finally:
        UF.set_compute_dtype(torch.bfloat16)
    (l0, s0, g0), (l1, s1, g1) = results
    assert torch.isfinite(l0) and torch.equal(l0, l1)
    assert all(torch.equal(s0[k], s1[k]) for k in s0)
    assert all(torch.equal(g0[k], g1[k]) for k in g0) and all(bool(torch.isfinite(v).all()) for v in g0.values())


def test_torchvision_state_dict_round_trips_through_ckpt_path_and_the_hooks(tmp_path):
    from src.models.baselines import classification as S
    from uia_hip import functional as UF
    R = case()
    src = {k: (v.float() if v.is_floating_point() else v + 5) for k, v in RR.seeded_state("resnet18", 1000, 99).items()}      # a 1000-class torchvision file
    path = tmp_path / "resnet18_tv.pth"
    torch.save(src, path)
    args = S.get_args(["--ckpt_path", str(path), "--device", "cuda:0", "--num_classes", "2"])
    try:
        UF.set_compute_dtype(torch.float32)
        net = S.prepare_model(args)
        sd = net.state_dict()
        assert all(torch.equal(sd[k].cpu(), v) for k, v in src.items() if not k.startswith("fc.")) and tuple(sd["fc.weight"].shape) == (2, 512)
        assert int(sd["layer4.1.bn2.num_batches_tracked"]) == 5
        net.eval()
        with torch.no_grad():
            a = net(R["x"].float().cuda())
        torch.save(net.checkpoint_dict(), tmp_path / "best_model.pth")
        other = S.prepare_model(S.get_args(["--device", "cuda:0", "--num_classes", "2", "--seed", "3"]))
        other.load_checkpoint(torch.load(tmp_path / "best_model.pth", map_location="cpu"))
        UF.WEIGHTS.bump()
        other.eval()
        with torch.no_grad():
            b = other(R["x"].float().cuda())
    finally:
        UF.set_compute_dtype(torch.bfloat16)
    assert list(other.state_dict()) == list(src) and torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_focal_loss_descends():
    """Four 64x64 images, two of each class, FlatAdapterOptimizer at lr 1e-2, 60 steps in train mode: the focal loss falls below half its
    start value."""
    from src.losses.focal import FocalLoss
    from src.third_party.resnet import resnet18
    from uia_hip import functional as UF
    from uia_hip.engine import FlatAdapterOptimizer, segmentation_step
    g = torch.Generator().manual_seed(1)
    x = torch.rand(4, 3, 64, 64, generator=g)
    labels = torch.tensor([0, 1, 0, 1]).cuda()
    try:
        UF.set_compute_dtype(torch.float32)
        torch.manual_seed(1)
        net = resnet18(num_classes=2).cuda()
        net.train()
        opt = FlatAdapterOptimizer(list(net.named_parameters()), lr=1e-2, betas=(0.9, 0.95), weight_decay=0.01, max_norm=0.0)
        crit = FocalLoss(to_onehot_y=True)
        xd = x.cuda()
        losses = [float(segmentation_step(net, crit, opt, xd, labels)[0]) for _ in range(60)]
    finally:
        UF.set_compute_dtype(torch.bfloat16)
    print("first", losses[0], "last four", losses[-4:])
    assert all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0], losses


def test_entry_point_end_to_end(tmp_path):
    import csv
    import glob
    import json
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "nextgen-uia_amd"), root]))
    base = [sys.executable, "-m", "src.models.baselines.classification", "--synthetic", "--synthetic_train", "8", "--synthetic_val", "4", "--synthetic_test", "4",
            "--img_size", "64", "--batch_size", "4", "--num_workers", "0"]
    r = subprocess.run(base + ["--epochs", "2", "--val_every", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    best = tmp_path / "runs" / "resnet_cls" / "LN-INT" / "train" / "best_model.pth"
    assert best.exists()
    state = torch.load(best, map_location="cpu")
    ref = json.load(open(os.path.join(HERE, "golden", "resnet18_keys.json")))["state"]
    assert [k for k in state] == [k for k, _ in ref] and tuple(state["fc.weight"].shape) == (2, 512)
    assert all(int(v) >= 2 for k, v in state.items() if k.endswith("num_batches_tracked"))
    r = subprocess.run(base + ["--test"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    found = glob.glob(str(tmp_path / "runs" / "resnet_cls" / "LN-INT" / "test" / "**" / "results.csv"), recursive=True)
    assert found
    rows = {r[0]: r[1:] for r in csv.reader(open(found[0]))}
    for key in ("Acc", "Rec", "Pre", "F1", "AUC"):
        assert key in rows and rows[key][0] != "" and np.isfinite(float(rows[key][0])), rows


def test_refusals_before_launch():
    from src.third_party.resnet import resnet18
    from uia_hip import functional as UF
    from uia_hip._lib import UiaError
    net = resnet18(num_classes=2).cuda()
    with pytest.raises(ValueError, match="smaller than 32"):
        net(torch.zeros(1, 3, 16, 16, device="cuda"))
    x = torch.zeros(1, 4, 4, 16, device="cuda", dtype=torch.bfloat16)
    bn = net.layer1[0].bn1
    args = (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, True, 0.1, 1e-5)
    before = bn.running_mean.clone()
    with pytest.raises(UiaError, match="not built"):
        UF.ConvBNReLUFn.apply(x, torch.zeros(64, 16, 5, 5, device="cuda"), *args, 1)
    with pytest.raises(UiaError, match="not built"):
        UF.ConvBNFn.apply(x, torch.zeros(64, 16, 3, 3, device="cuda"), *args, 3)
    with pytest.raises(UiaError, match="residual"):
        UF.ConvBNAddReLUFn.apply(x, torch.zeros(1, 4, 4, 32, device="cuda", dtype=torch.bfloat16), torch.zeros(64, 16, 3, 3, device="cuda"), *args, 1)
    with pytest.raises(UiaError, match="channels"):
        UF.ConvBNReLUFn.apply(x, torch.zeros(64, 32, 3, 3, device="cuda"), *args, 1)
    torch.cuda.synchronize()
    assert torch.equal(bn.running_mean, before) and int(bn.num_batches_tracked) == 0
