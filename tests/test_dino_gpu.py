"""-m gpu: the DINOv2 classifier on the HIP path.  Golden parity of the small geometry (577 tokens: every attention is uia_attn_fwd_long) against the
reference's recorded outputs, the full ViT-B/14 at 518 px against the float64 restatement (tests/dino_reference.py), the entry point end to end in a
child process, descent of the focal loss, the patch-mean pool kernel, and the refusal of a training request past the attention backward's 272 tokens.
Bars: the project's (max |error| / max |reference| per tensor): 1e-3 in fp32, 1e-2 in bf16."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dino_reference as DR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BARS = {torch.float32: 1e-3, torch.bfloat16: 1e-2}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def small_model(device="cuda"):
    from src.models.dino.classification import build_model
    S = DR.SMALL
    torch.manual_seed(0)
    m = build_model(S["img_size"], S["patch_size"], S["num_classes"], depth=S["depth"], embed_dim=S["embed_dim"], num_heads=S["num_heads"])
    state = DR.seeded_state(S["img_size"], S["patch_size"], S["embed_dim"], S["depth"], S["num_classes"], S["seed"])
    m.feature_model.load_state_dict({k: v for k, v in state.items() if k.startswith("encoder.")})
    m.classifier.load_state_dict({k: v for k, v in state.items() if k.startswith("linear.")})
    return m.to(device), state


@pytest.fixture
def dtype_guard():
    from uia_hip import functional as UF
    yield UF
    UF.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16))
def test_small_golden_parity(dtype_guard, dt):
    UF = dtype_guard
    UF.set_compute_dtype(dt)
    S = DR.SMALL
    z = np.load(os.path.join(HERE, "golden", "dino_small.npz"))
    m, _ = small_model()
    m.eval()
    images = DR.seeded_images(S["batch"], S["img_size"], S["seed"]).cuda()
    with torch.no_grad():
        feats = m.feature_model(images)
        logits = m.classifier(feats)
    torch.cuda.synchronize()
    ef, el = rel(feats, torch.from_numpy(z["features"])), rel(logits, torch.from_numpy(z["logits"]))
    print(f"small DINOv2 {dt}: features {ef:.2e}, logits {el:.2e}")
    assert ef <= BARS[dt] and el <= BARS[dt], (ef, el)


@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16))
def test_full_geometry_vitb14_518(dtype_guard, dt):
    """ViT-B/14 at 518 px (1370 tokens), B = 2, seeded weights: features and logits against the float64 restatement."""
    from src.models.dino.classification import build_model
    UF = dtype_guard
    UF.set_compute_dtype(dt)
    torch.manual_seed(0)
    m = build_model(518, 14, 2)
    state = DR.seeded_state(518, 14, 768, 12, 2, seed=77)
    m.feature_model.load_state_dict({k: v for k, v in state.items() if k.startswith("encoder.")})
    m.classifier.load_state_dict({k: v for k, v in state.items() if k.startswith("linear.")})
    m = m.cuda().eval()
    images = DR.seeded_images(2, 518, 77).cuda()
    with torch.no_grad():
        feats = m.feature_model(images)
        logits = m.classifier(feats)
    f64, l64 = DR.forward(images, state, 12, 14, device=torch.device("cuda"))
    ef, el = rel(feats, f64), rel(logits, l64)
    print(f"ViT-B/14 518 {dt}: features {ef:.2e}, logits {el:.2e}")
    assert feats.shape == (2, 3840) and torch.isfinite(feats).all()
    assert ef <= BARS[dt] and el <= BARS[dt], (ef, el)


def test_patch_mean_pool_kernel():
    """ops.ln_mean_rows against LayerNorm + mean in float64; two runs bit-identical; odd row ranges and a strided output."""
    from uia_hip import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    for B, L, D, r0, n in ((3, 1370, 768, 1, 1369), (2, 577, 128, 1, 576), (1, 5, 384, 2, 3), (2, 40, 1024, 0, 40)):
        x = torch.randn(B, L, D, device="cuda", generator=g) * 2 + 0.5
        w = torch.randn(D, device="cuda", generator=g) * 0.1 + 1
        b = torch.randn(D, device="cuda", generator=g) * 0.1
        out = torch.full((B, D + 12), float("nan"), device="cuda")
        ops.ln_mean_rows(x, w, b, 1e-6, r0, n, out=out[:, 4:4 + D])
        again = ops.ln_mean_rows(x, w, b, 1e-6, r0, n)
        ref = torch.nn.functional.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-6)[:, r0:r0 + n].mean(1)
        assert rel(out[:, 4:4 + D], ref) < 1e-5, (B, L, D)
        assert torch.equal(out[:, 4:4 + D], again)
        assert torch.isnan(out[:, :4]).all() and torch.isnan(out[:, 4 + D:]).all()


def test_training_request_past_272_tokens_is_refused():
    from uia_hip._lib import UiaError
    m, _ = small_model()
    blk = m.feature_model.encoder.blocks[0][0]
    x = torch.randn(2, 577, DR.SMALL["embed_dim"], device="cuda", requires_grad=True)
    with pytest.raises(UiaError, match="272"):
        blk(x)


def test_focal_loss_descends():
    """The head alone trains on frozen features of learnable synthetic images (class 1 carries a bright ellipse): the focal loss falls."""
    from src.datasets.classification import synthetic_split
    from src.losses.focal import FocalLoss
    from uia_hip.engine import FlatAdapterOptimizer, segmentation_step
    m, _ = small_model()
    m.train()
    images, labels = synthetic_split(16, DR.SMALL["img_size"], seed=3)
    images, labels = images.cuda(), labels.cuda()
    opt = FlatAdapterOptimizer([(n, p) for n, p in m.named_parameters() if p.requires_grad], lr=3e-3, betas=(0.9, 0.95), weight_decay=0.01, max_norm=0.0)
    crit = FocalLoss(to_onehot_y=True)
    losses = [float(segmentation_step(m, crit, opt, images, labels, lr=3e-3)[0]) for _ in range(40)]
    print("focal loss", losses[0], min(losses[-4:]))
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["classifier.linear.weight", "classifier.linear.bias"]
    assert min(losses[-4:]) < 0.8 * losses[0], losses


def test_entry_point_end_to_end(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "nextgen-uia_amd"), ROOT]))
    cmd = [sys.executable, "-m", "src.models.dino.classification", "--synthetic", "--epochs", "2", "--val_every", "1", "--synthetic_train", "48",
           "--synthetic_val", "24", "--synthetic_test", "24", "--batch_size", "8", "--num_workers", "0"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    best = tmp_path / "runs" / "dino_cls" / "LN-INT" / "train" / "best_model.pth"
    assert best.exists()
    state = torch.load(best, map_location="cpu")
    assert sorted(state) == ["linear.bias", "linear.weight"] and tuple(state["linear.weight"].shape) == (2, 3840)
    from src.third_party.dino.dinov2 import ClassificationHead
    head = ClassificationHead(768, 2, 4)
    head.load_state_dict(state)
    assert glob.glob(str(tmp_path / "runs" / "dino_cls" / "LN-INT" / "test" / "**" / "results.csv"), recursive=True)
