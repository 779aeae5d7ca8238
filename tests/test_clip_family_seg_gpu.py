"""-m gpu: the three CLIP-family segmentation entries (src.models.{clip,metaclip,unimedclip}.segmentation) at toy geometry — the command line end to end
(train, the four-key checkpoint, test, --test alone, the pictures), a Mona checkpoint of the family's own fine-tune entry (and, for clip, a LoRA one), and
the parity of the model each entry builds with the float64 restatement of its tower (oracle/vit_ref.py, as the family's classification / fine-tune parity
tests use it) with the feature-pyramid seg head restated beside it.

Bars are the project's: fp32 1e-3 on the logits and on every trainable gradient against the global gradient scale; bf16 max(1e-2, 2 x e_ref) with e_ref the
error of the same restatement run in torch.bfloat16 on the CPU (tests/test_unet_baseline_gpu.py)."""
import importlib
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu
FAMILIES = ["clip", "metaclip", "unimedclip"]
# the tiny towers of tests/test_classification_gpu.py's CLI test, at 64 pixels a side (an 8 x 8 grid of 8-pixel patches)
CONFIG = {"clip": repr((64, 64, 2, 128, 8, 16, 100, 128, 2, 2)),
          "metaclip": repr(dict(embed_dim=64, vision_cfg=dict(img_size=64, patch_size=8, embed_dim=128, depth=2, num_heads=2, mlp_ratio=2.0, eps=1e-5,
                                                             act="quick_gelu", pre_norm=True, patch_bias=False),
                                text_cfg=dict(context_length=16, vocab_size=100, width=64, heads=1, layers=1, act="quick_gelu"))),
          "unimedclip": repr(dict(embed_dim=64, image_size=64, vision_layers=2, vision_width=128, patch_size=8, context_length=16, vocab_size=100,
                                  width=64, heads=1, layers=1))}
HEADS = {"clip": 2, "metaclip": 2, "unimedclip": 2}             # vision heads: width 128 / 64 per head
TOY = ["--synthetic", "--img_size", "64", "--patch_size", "8", "--reduce_dim", "64", "--batch_size", "4", "--synthetic_train", "8", "--synthetic_val", "4",
       "--synthetic_test", "5", "--device", "cuda:0", "--num_workers", "0", "--extract_layers", "0,1"]
BAR32, BAR16 = 1e-3, 1e-2


def dev():
    return torch.device("cuda:0")


def argv_of(family, *more):
    ckpt = [] if family == "metaclip" else ["--ckpt", "absent.pt"]
    return TOY + ["--model_config", CONFIG[family]] + ckpt + list(more)


def cli_of(family):
    return importlib.import_module(f"src.models.{family}.segmentation")


def backups(exp):
    root = f"runs/{exp}/LN-INT/test"
    return [os.path.join(root, d) for d in sorted(os.listdir(root)) if "_iou=" in d]


def finetune_checkpoint(family, where):
    """best_model.pth of the family's own fine-tune entry (Mona, the family's default variant noise_aware) at the toy geometry."""
    ft = importlib.import_module(f"src.models.{family}.finetune")
    cwd = os.getcwd()
    os.chdir(where)
    try:
        extra = {"clip": ["--ckpt", ""], "metaclip": [], "unimedclip": ["--num_workers", "0"]}[family]
        ft.main(["--synthetic", "--synthetic_train", "16", "--synthetic_val", "8", "--img_size", "64", "--batch_size", "8", "--epochs", "1", "--lr", "2e-3",
                 "--dtype", "bf16", "--exp", "ft", "--model_config", CONFIG[family]] + extra)
    finally:
        os.chdir(cwd)
    path = os.path.join(where, "runs", "ft", "best_model.pth")
    assert os.path.exists(path)
    return path


# ------------------------------------------------------------------------------------------------ the command line
@pytest.mark.parametrize("family", FAMILIES)
def test_entry_trains_checkpoints_tests_and_draws(tmp_path, monkeypatch, family):
    cli = cli_of(family)
    monkeypatch.chdir(tmp_path)
    out = cli.main(argv_of(family, "--epochs", "2", "--val_every", "1", "--exp", family, "--dtype", "fp32"))
    assert out["iters"] == 4 and math.isfinite(out["last_loss"]) and 0.0 <= out["best_val_dice"] <= 1.0 and math.isfinite(out["test"]["loss"])
    ck = torch.load(f"runs/{family}/LN-INT/train/best_model.pth", map_location="cpu")
    assert set(ck) == {"reduces", "blocks", "seg_head", "mona"} and ck["mona"] == {}
    assert set(ck["seg_head"]) == {"1.weight", "1.bias"} and "0.weight" in ck["reduces"] and "1.3.bias" in ck["blocks"]
    (folder,) = backups(family)
    assert sorted(os.listdir(os.path.join(folder, "viz"))) == sorted(f"test_{i:05d}{t}.png" for i in range(5) for t in ("", "_overlay", "_pred"))
    rows = [line.split(",") for line in open(out["test"]["results_csv"]).read().strip().splitlines()]
    assert rows[0] == ["Metric", "Mean", "Std"] and [r[0] for r in rows[1:]] == ["Dice", "IoU", "HD95", "ASD"]
    again = cli.main(argv_of(family, "--exp", family, "--dtype", "fp32", "--test"))
    assert set(again) == {"test"} and len(backups(family)) == 2
    assert open(again["test"]["results_csv"], "rb").read() == open(out["test"]["results_csv"], "rb").read()


def trainable_gradients(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    model.eval()
    out = model(torch.rand(2, 3, 64, 64, generator=g).to(dev()))
    assert tuple(out.shape) == (2, 2, 64, 64) and out.dtype == torch.float32 and out.is_contiguous()
    (out * torch.randn(out.shape, generator=g).to(dev())).sum().backward()
    return {k: p.grad for k, p in model.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("family", FAMILIES)
def test_mona_checkpoint_of_the_finetune_entry_is_loaded_and_trained(tmp_path, monkeypatch, family):
    from uia_hip import functional as UF
    cli = cli_of(family)
    ckpt = finetune_checkpoint(family, str(tmp_path))
    saved = torch.load(ckpt, map_location="cpu")
    assert saved and all("mona" in k for k in saved)
    monkeypatch.chdir(tmp_path)
    UF.set_compute_dtype(torch.float32)
    try:
        args = cli.get_args(argv_of(family, "--mona_weights", ckpt))
        loaded, real = [], cli.load_adapter_by_name
        monkeypatch.setattr(cli, "load_adapter_by_name", lambda *a: loaded.append((a[2], real(*a))) or loaded[-1][1])
        model = cli.prepare_model(args)
        assert loaded == [("mona_state_dict", len(saved))] and len(saved) > 0        # the entry's own count of tensors loaded by name
        sd = model.clip_model.state_dict()
        assert all(torch.equal(sd[k].cpu(), v) for k, v in saved.items())
        grads = trainable_gradients(model)
        received = sorted(k for k, v in grads.items() if v is not None)           # the unused cls_head stays trainable and receives nothing, as in the reference
        assert received and all(("mona" in k and k.startswith("clip_model.")) or k.startswith(("reduces.", "blocks.", "seg_head.")) for k in received), received
        assert sum("mona" in k for k in grads) == len(saved) and sum("mona" in k for k in received) > 0
        assert not any(p.requires_grad for k, p in model.named_parameters() if k.startswith("clip_model.") and "mona" not in k)
        reached = [k for k, v in grads.items() if v is not None and float(v.abs().max()) > 0.0]
        assert any("mona" in k for k in reached) and any(k.startswith("seg_head.") for k in reached) and any(k.startswith("reduces.") for k in reached)
        ck = model.checkpoint_dict()
        assert set(ck) == {"reduces", "blocks", "seg_head", "mona"} and len(ck["mona"]) == len(saved)
    finally:
        UF.set_compute_dtype(torch.bfloat16)


def test_clip_takes_a_lora_checkpoint_by_its_adapter_type(tmp_path, monkeypatch):
    from src.adapters import inject_lora_to_clip
    from src.models.clip import segmentation as cli
    from src.models.clip.finetune import _geometry
    from src.third_party.openai_clip.model import load_clip
    from uia_hip import functional as UF
    monkeypatch.chdir(tmp_path)
    args = cli.get_args(argv_of("clip"))
    donor = load_clip(args.ckpt_path or args.ckpt, _geometry(args), args.seed)
    inject_lora_to_clip(donor, lora_r=4, lora_alpha=8, lora_dropout=0.0)
    g = torch.Generator().manual_seed(2)
    state = {k: 0.05 * torch.randn(v.shape, generator=g) for k, v in donor.state_dict().items() if "lora" in k}
    assert state
    torch.save({"adapter_type": "lora", "lora_r": 4, "lora_alpha": 8, "lora_dropout": 0.0, "lora_state_dict": state}, "lora.pth")
    UF.set_compute_dtype(torch.float32)
    try:
        loaded, real = [], cli.load_adapter_by_name
        monkeypatch.setattr(cli, "load_adapter_by_name", lambda *a: loaded.append((a[2], real(*a))) or loaded[-1][1])
        model = cli.prepare_model(cli.get_args(argv_of("clip", "--mona_weights", "lora.pth")))
        assert loaded == [("lora_state_dict", len(state))]
        sd = model.clip_model.state_dict()
        assert all(torch.equal(sd[k].cpu(), v) for k, v in state.items()) and not any("mona" in k for k in sd)
        grads = trainable_gradients(model)
        assert any(k.startswith("seg_head.") for k in grads) and all(torch.isfinite(v).all() for v in grads.values() if v is not None)
    finally:
        UF.set_compute_dtype(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ parity of the model an entry builds
def fpn_seg_head(acts, A, img_size):
    """FPNAdapter.forward for task="seg", restated (reference src/third_party/timm/clip_adapter.py: reduce -> LayerNorm -> Linear -> GELU -> Linear per
    level, summed deep to shallow, bilinear upsample, Conv1x1): acts are the tapped tokens [B, 1 + n, D], A the adapter's own state dict."""
    a = None
    for lvl in range(len(acts) - 1, -1, -1):
        r = F.linear(acts[lvl][:, 1:, :], A[f"reduces.{lvl}.weight"], A[f"reduces.{lvl}.bias"])
        h = F.layer_norm(r, (r.shape[-1],), A[f"blocks.{lvl}.0.weight"], A[f"blocks.{lvl}.0.bias"], 1e-5)
        h = F.gelu(F.linear(h, A[f"blocks.{lvl}.1.weight"], A[f"blocks.{lvl}.1.bias"]))
        h = F.linear(h, A[f"blocks.{lvl}.3.weight"], A[f"blocks.{lvl}.3.bias"])
        a = h if a is None else h + a
    B, n, C = a.shape
    g = int(math.sqrt(n))
    up = F.interpolate(a.permute(0, 2, 1).reshape(B, C, g, g), size=(img_size, img_size), mode="bilinear", align_corners=False)
    return F.conv2d(up, A["seg_head.1.weight"], A["seg_head.1.bias"])


def restated(family, images, P, A, layers=(0, 1), img_size=64):
    """P: the tower's state dict under the names the oracle reads (the native tower's Mona wrapper names mapped to the OpenAI ones)."""
    from oracle import vit_ref
    mona = dict(variant="noise_aware", hw=(8, 8), keep_masks=None, p_drop=0.0)
    if family == "metaclip":
        taps = {"layers": list(layers), "acts": []}
        vit_ref.timm_vit_forward(images, P, heads=HEADS[family], mona=mona, taps=taps, return_tokens=True, eps=1e-5, act="quick_gelu")
        acts = taps["acts"]
    else:
        _, acts = vit_ref.openai_vit_forward(images, P, heads=HEADS[family], mona=mona, taps=list(layers))
    return fpn_seg_head(acts, A, img_size)


def oracle_name(family, k):
    return k.replace(".mona.clip_mona.", ".mona.") if family == "unimedclip" else k


def restated_run(family, sd, names, images, dy, dtype):
    """Logits and the gradients of `names` from the restatement in `dtype` on the CPU."""
    cast = lambda v: v.detach().to(dtype) if v.is_floating_point() else v.detach().clone()
    leaves = {k: cast(sd[k]).clone().requires_grad_(True) for k in names}
    full = {k: leaves.get(k, None) if k in leaves else cast(v) for k, v in sd.items()}
    P = {oracle_name(family, k[len("clip_model."):]): v for k, v in full.items() if k.startswith("clip_model.")}
    A = {k: v for k, v in full.items() if not k.startswith("clip_model.")}
    out = restated(family, images.to(dtype), P, A)
    (out * dy.to(dtype)).sum().backward()
    return out.detach().double(), {k: (v.grad.detach().double() if v.grad is not None else None) for k, v in leaves.items()}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(scope="module")
def mona_checkpoints(tmp_path_factory):
    """Per family a Mona state (the names an injected tower has, values N(0, 0.05) around the identity of the norms) as a --mona_weights file."""
    made = {}

    def get(family):
        if family not in made:
            from src.adapters import inject_mona_variant_to_clip, inject_mona_variant_to_open_clip
            cli = cli_of(family)
            where = tmp_path_factory.mktemp(f"mona_{family}")
            cwd = os.getcwd()
            os.chdir(where)
            try:
                tower = cli.prepare_model(cli.get_args(argv_of(family, "--device", "cpu"))).clip_model
            finally:
                os.chdir(cwd)
            (inject_mona_variant_to_clip if family == "clip" else inject_mona_variant_to_open_clip)(tower, variant="noise_aware", bottleneck_dim=64)
            g = torch.Generator().manual_seed(11)
            state = {k: (0.05 * torch.randn(v.shape, generator=g) + (1.0 if k.endswith(("norm.weight", "gammax")) else 0.0)) for k, v in tower.state_dict().items()
                     if "mona" in k and v.is_floating_point()}
            path = os.path.join(where, "mona.pth")
            torch.save(state, path)
            made[family] = path
        return made[family]
    return get


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_model_of_the_entry_against_the_float64_restatement(family, mode, mona_checkpoints, tmp_path, monkeypatch):
    from uia_hip import functional as UF
    cli = cli_of(family)
    monkeypatch.chdir(tmp_path)
    UF.set_compute_dtype(torch.float32 if mode == "fp32" else torch.bfloat16)
    try:
        model = cli.prepare_model(cli.get_args(argv_of(family, "--mona_weights", mona_checkpoints(family), "--device", "cpu")))
        g = torch.Generator().manual_seed(21)
        with torch.no_grad():                                    # heads away from their initial values: every level of the pyramid carries weight
            for k, p in model.named_parameters():
                if k.startswith(("reduces.", "blocks.", "seg_head.")):
                    p.add_(0.02 * torch.randn(p.shape, generator=g))
        model.eval()
        names = [k for k, p in model.named_parameters() if p.requires_grad]
        assert any("mona" in k for k in names) and any(k.startswith("seg_head.") for k in names)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        images = torch.rand(2, 3, 64, 64, generator=g)
        dy = torch.randn(2, 2, 64, 64, generator=g)
        want, want_g = restated_run(family, sd, names, images, dy, torch.float64)
        model = model.to(dev())
        out = model(images.to(dev()))
        (out * dy.to(dev())).sum().backward()
        got_g = {k: p.grad for k, p in model.named_parameters() if p.requires_grad}
        gscale = max(float(v.abs().max()) for v in want_g.values() if v is not None)

        def grad_errors(gr):
            errs = {}
            for k in names:
                if want_g[k] is None:                            # a parameter the loss does not reach
                    assert gr[k] is None or float(gr[k].abs().max()) == 0.0, k
                    continue
                errs[k] = float((gr[k].detach().double().cpu() - want_g[k]).abs().max()) / gscale
            return errs

        e_out, e_grad = rel(out, want), grad_errors(got_g)
        worst = max(e_grad, key=e_grad.get)
        if mode == "fp32":
            print(f"{family} fp32: logits {e_out:.2e}, worst gradient {e_grad[worst]:.2e} ({worst}) of {len(e_grad)}")
            assert e_out <= BAR32 and e_grad[worst] <= BAR32, (e_out, worst, e_grad[worst])
        else:
            ref16, ref16_g = restated_run(family, sd, names, images, dy, torch.bfloat16)
            r_out, r_grad = rel(ref16, want), grad_errors(ref16_g)
            r_worst = max(r_grad.values())
            print(f"{family} bf16: logits {e_out:.2e} (e_ref {r_out:.2e}), worst gradient {e_grad[worst]:.2e} ({worst}; e_ref {r_worst:.2e})")
            assert e_out <= max(BAR16, 2.0 * r_out), (e_out, r_out)
            assert e_grad[worst] <= max(BAR16, 2.0 * r_worst), (worst, e_grad[worst], r_worst)
    finally:
        UF.set_compute_dtype(torch.bfloat16)
