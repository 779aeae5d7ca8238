"""CPU: the DINOv2 UNet segmentation decoder's module surface against the reference's (tests/golden/dino_seg_keys.json, written by
tools/gen_dino_seg_golden.py from the imported reference), its refusals, and the float64 restatement of tests/unet_reference.py against the
reference's recorded outputs (dino_seg_small.npz)."""
import json
import os

import numpy as np
import pytest
import torch

import unet_reference as UR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def test_state_dict_names_match_reference():
    from src.third_party.dino.dinov2 import setup_decoders
    ref = json.load(open(os.path.join(GOLDEN, "dino_seg_keys.json")))
    decoders, groups = setup_decoders(768, [1e-4], num_classes=2, decoder_type="unet", image_size=518, patch_size=14)
    assert list(decoders.decoders_dict.keys()) == ref["module_keys"] == ["unet:lr=0_0001000000"]
    got = [[k, list(v.shape)] for k, v in decoders.state_dict().items()]
    assert got == ref["state"]
    assert any(k.endswith("conv.1.num_batches_tracked") for k, _ in got)
    assert len(groups) == 1 and groups[0]["lr"] == 1e-4
    # a reference-named state dict loads strictly, and ours loads into the same names
    sd = {k: torch.zeros(s, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, s in ref["state"]}
    decoders.load_state_dict(sd, strict=True)


def test_restatement_names_match_reference_order():
    ref = json.load(open(os.path.join(GOLDEN, "dino_seg_keys.json")))
    prefix = ref["module_keys"][0]
    want = [[k[len("decoders_dict.") + len(prefix) + 1:], s] for k, s in ref["state"]]
    assert want == [[k, list(s)] for k, s in UR.state_shapes(768, 2)]


@pytest.mark.parametrize("kind", ["linear", "segformer"])
def test_non_unet_decoders_are_refused(kind):
    from src.third_party.dino.dinov2 import setup_decoders
    with pytest.raises(ValueError, match="only 'unet' runs"):
        setup_decoders(768, [1e-4], num_classes=2, decoder_type=kind, image_size=518, patch_size=14)


def test_wrong_map_count_and_shape_are_refused():
    from src.third_party.dino.dinov2 import UNetDecoder
    dec = UNetDecoder(64, 3, image_size=84, resize_image=True, patch_size=14)
    with pytest.raises(ValueError, match="last 5 blocks"):
        dec([torch.zeros(1, 36, 64)] * 4)
    with pytest.raises(ValueError, match="patch tokens"):
        dec([torch.zeros(1, 37, 64)] * 5)


def test_restatement_reproduces_reference_golden():
    S = UR.SMALL
    g = np.load(os.path.join(GOLDEN, "dino_seg_small.npz"))
    P = UR.seeded_state(S["embed_dim"], S["num_classes"], S["seed"])
    maps, dlogits = UR.seeded_inputs(**S)
    names = [k for k, _ in UR.state_shapes(S["embed_dim"], S["num_classes"]) if "running" not in k and "num_batches" not in k]
    for k in names:
        P[k].requires_grad_(True)
    out, bufs = UR.decoder_forward(P, maps, S["image_size"], S["patch_size"], training=True)

    def rel(a, b, floor=0.0):
        b = torch.as_tensor(b, dtype=torch.float64)
        return float((a.detach() - b).abs().max() / max(float(b.abs().max()), floor))

    assert rel(out, g["train_out"]) < 1e-6
    (out * dlogits).sum().backward()
    for k in names:
        # the biases of convs followed by train-mode BatchNorm have a zero gradient: measured against 1e-6 there
        assert rel(P[k].grad, g["grad:" + k], floor=1e-6) < 1e-5, k
    for k, v in bufs.items():
        if v.dtype == torch.int64:
            assert int(v) == int(g["buf:" + k]) == 1, k
        else:
            assert rel(v, g["buf:" + k]) < 1e-6, k
    Pe = {k: v.detach() for k, v in P.items()}
    with torch.no_grad():
        ev, _ = UR.decoder_forward(Pe, maps, S["image_size"], S["patch_size"], training=False, bufs=bufs)
    assert rel(ev, g["eval_out"]) < 1e-6
    # the reference quirk: logits pass BN + ReLU before the resize, so the resize's overshoot can go below zero
    assert float(out.detach().min()) < 0.0 < float(out.detach().max())


def test_cli_table_matches_reference():
    import ast
    from oracle.gen_host_fixtures import argparse_table
    from src.models.dino import segmentation as S
    ref = json.load(open(os.path.join(GOLDEN, "reference_dino_seg_cli_table.json")))
    assert "--decoder_type" in ref and len(ref) >= 20
    got = argparse_table(os.path.join(os.path.dirname(HERE), "nextgen-uia_amd/src/models/dino/segmentation.py"))
    args = vars(S.get_args([]))
    for flag, kw in ref.items():
        assert flag in got, flag
        if flag == "--device":
            continue
        assert got[flag] == kw, (flag, kw, got[flag])
        if "default" in kw:
            assert args[flag[2:]] == ast.literal_eval(kw["default"]), flag
    for flag in ("--dtype", "--synthetic", "--synthetic_train", "--data_pt", "--ckpt_path", "--stats_json", "--val_every"):
        assert flag[2:] in args, flag
    assert args["img_size"] == 518 and args["batch_size"] == 24 and args["exp"] == "dino_seg" and args["decoder_type"] == "unet"


@pytest.mark.parametrize("argv, match", [(["--decoder_type", "linear"], "only 'unet' runs"), (["--img_size", "500"], "not a multiple")])
def test_entry_point_refuses_before_allocation(argv, match):
    from src.models.dino import segmentation as S
    with pytest.raises(ValueError, match=match):
        S.main(argv + ["--synthetic", "--device", "cpu"])


@pytest.mark.parametrize("n", [2, 3, 6])
def test_encoder_refuses_other_block_counts(n):
    from src.third_party.dino import vision_transformer as vit
    from src.third_party.dino.dinov2 import DINOV2Encoder
    with pytest.raises(ValueError, match="Unsupported number of layers"):
        DINOV2Encoder(vit.DinoVisionTransformer(img_size=28, patch_size=14, embed_dim=64, depth=6, num_heads=1), n_last_blocks=n)


def test_checkpoint_is_the_decoders_state_dict():
    from src.models.dino.segmentation import build_model
    ref = json.load(open(os.path.join(GOLDEN, "dino_seg_keys.json")))
    model = build_model(img_size=518, patch_size=14, num_classes=2, depth=1)
    state = model.checkpoint_dict()
    assert [[k, list(v.shape)] for k, v in state.items()] == ref["state"]
    assert not any(p.requires_grad for p in model.feature_model.parameters())
    assert all(p.requires_grad for p in model.decoders.parameters())
    model.load_checkpoint({k: v.clone() for k, v in state.items() if "num_batches" not in k})     # strict=False, as the reference
    model.train()
    assert model.decoders.training and not model.feature_model.training
