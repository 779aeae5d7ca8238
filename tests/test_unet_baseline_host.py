"""CPU: the UNet baseline's module surface and command line against the reference's (tests/golden/unet_baseline_keys.json and
reference_baseline_seg_cli_table.json, written by tools/gen_unet_baseline_golden.py from the imported reference), the float64 restatement of
tests/unet_baseline_reference.py against the reference's recorded outputs (unet_baseline_small.npz + unet_baseline_small_down4.npz), the
refusals, and which kernel form every convolution launch of the model takes (uia_conv_igemm_form / uia_conv_wgrad_form: no GPU needed)."""
import json
import os

import numpy as np
import pytest
import torch

import unet_baseline_reference as UB
import unet_reference as UR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def golden_small():
    g = dict(np.load(os.path.join(GOLDEN, "unet_baseline_small.npz")))
    g.update(np.load(os.path.join(GOLDEN, "unet_baseline_small_down4.npz")))
    return g


def test_cli_table_matches_reference():
    import ast
    from oracle.gen_host_fixtures import argparse_table
    from src.models.baselines import segmentation as S
    ref = json.load(open(os.path.join(GOLDEN, "reference_baseline_seg_cli_table.json")))
    assert "--patience" in ref and len(ref) >= 19
    got = argparse_table(os.path.join(os.path.dirname(HERE), "nextgen-uia_amd/src/models/baselines/segmentation.py"))
    args = vars(S.get_args([]))
    for flag, kw in ref.items():
        assert flag in got, flag
        if flag == "--device":
            continue
        assert got[flag] == kw, (flag, kw, got[flag])
        if "default" in kw:
            assert args[flag[2:]] == ast.literal_eval(kw["default"]), flag
    for flag in ("--dtype", "--synthetic", "--synthetic_train", "--data_pt", "--stats_json", "--val_every"):
        assert flag[2:] in args, flag
    assert (args["exp"], args["img_size"], args["batch_size"], args["lr"], args["beta1"], args["beta2"], args["weight_decay"], args["patience"]) == \
        ("unet_seg", 224, 32, 1e-4, 0.9, 0.95, 0.01, 15)


def test_state_dict_names_match_reference():
    from src.third_party.unet import UNet
    ref = json.load(open(os.path.join(GOLDEN, "unet_baseline_keys.json")))["state"]
    net = UNet(3, 2)
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == ref
    assert got == [[k, list(s)] for k, s in UB.state_shapes(3, 2, 16)]
    assert sum(k.endswith("num_batches_tracked") for k, _ in got) == 18
    sd = {k: torch.zeros(s, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, s in ref}
    net.load_state_dict(sd, strict=True)
    assert list(net.checkpoint_dict().keys()) == [k for k, _ in ref]
    # the reference's dropout rates: the encoder's five blocks, none in the decoder
    drops = [m.p for m in net.encoder.modules() if isinstance(m, torch.nn.Dropout)]
    assert drops == [0.05, 0.1, 0.2, 0.3, 0.5] and all(m.p == 0.0 for m in net.decoder.modules() if isinstance(m, torch.nn.Dropout))
    assert all(u.bilinear for u in (net.decoder.up1, net.decoder.up2, net.decoder.up3, net.decoder.up4))


def test_transposed_upblock_keeps_the_reference_names():
    from src.third_party.unet import UpBlock
    keys = list(UpBlock(32, 16, 16, 0.0, bilinear=False).state_dict().keys())
    assert keys[:2] == ["up.weight", "up.bias"] and "conv1x1.weight" not in keys


def test_restatement_reproduces_reference_golden():
    S = UB.SMALL
    g = golden_small()
    P = UB.seeded_state(S["in_channels"], S["num_classes"], S["init_channels"], S["seed"])
    x, dlogits = UB.seeded_inputs(**S)
    masks = UB.seeded_masks(**S)
    out, bufs, grads, ev = UB.run_restatement(P, x, masks, dlogits, torch.float64)

    def rel(a, b, floor=0.0):
        b = torch.as_tensor(b, dtype=torch.float64)
        return float((a - b).abs().max() / max(float(b.abs().max()), floor))

    assert rel(out, g["train_out"]) < 1e-6
    assert len(grads) == sum(1 for k in g if k.startswith("grad:"))
    for k, v in grads.items():
        # the biases of convs followed by train-mode BatchNorm have a zero gradient: measured against 1e-6 there
        assert rel(v, g["grad:" + k], floor=1e-6) < 1e-6, k
    for k, v in bufs.items():
        if v.dtype == torch.int64:
            assert int(v) == int(g["buf:" + k]) == 1, k
        else:
            assert rel(v, g["buf:" + k]) < 1e-6, k
    assert rel(ev, g["eval_out"]) < 1e-6
    for f in ("unet_baseline_small.npz", "unet_baseline_small_down4.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, f)) < (1 << 20), f


def test_one_channel_restatement_equals_three_equal_channels():
    S = UB.SMALL
    P = UB.seeded_state(S["in_channels"], S["num_classes"], S["init_channels"], S["seed"])
    x, _ = UB.seeded_inputs(**S)
    a, _ = UB.unet_forward(P, x[:, :1], None, training=False)
    b, _ = UB.unet_forward(P, x[:, :1].repeat(1, 3, 1, 1), None, training=False)
    assert torch.equal(a, b)


def test_kernel_form_of_every_conv_launch():
    """Every conv launch of UNet(3, 2, 16) takes the matrix-core kernel, except those that touch the 3-channel input or the 2-channel output."""
    from uia_hip import ops
    direct = {"encoder.in_conv.0 forward", "encoder.in_conv.0 wgrad", "decoder.out_conv forward", "decoder.out_conv dgrad", "decoder.out_conv wgrad"}
    launches = UB.conv_launches(3, 2, 16)
    assert len(launches) == 18 * 3 - 1 + 4 * 3 + 3
    seen = set()
    for name, kind, mode, c1, c2, n, n1 in launches:
        form = ops.conv_igemm_form(mode, c1, c2, n, n1) if kind == "igemm" else ops.conv_wgrad_form(mode, c1, c2, n)
        assert form == (0 if name in direct else 1), (name, kind, mode, c1, c2, n, n1, form)
        seen.add(name)
    assert direct <= seen
    # the shapes that took the MFMA kernel before still do; the direct ones of the existing contract test still are
    for B, H, W, c1, c2, n in UR.CONV_MFMA:
        assert ops.conv_igemm_form(ops.CONV3, c1, c2, n) == 1
        assert ops.conv_igemm_form(ops.CONV3, n, 0, c1 + c2, c1) == (1 if n % 8 == 0 else 0)      # the data gradient reads the N channels of dy
        assert ops.conv_wgrad_form(ops.CONV3, c1, c2, n) == (1 if n % 8 == 0 else 0)
    assert ops.conv_igemm_form(ops.CONV3, 33, 0, 5) == 0 and ops.conv_wgrad_form(ops.CONV3, 33, 0, 5) == 0
    assert ops.conv_igemm_form(ops.CONV3, 34, 30, 32) == 0 and ops.conv_wgrad_form(ops.CONV3, 34, 30, 32) == 0
    assert ops.conv_igemm_form(ops.CONV3, 4, 6, 2) == 0 and ops.conv_igemm_form(ops.CONV3, 32, 0, 3) == 0
    assert ops.conv_igemm_form(ops.CONV1, 3, 0, 2) == 0 and ops.conv_igemm_form(ops.CONV1, 24, 0, 8) == 1
    assert ops.conv_igemm_form(ops.CONVT_FWD, 16, 0, 32) == 1 and ops.conv_igemm_form(ops.CONVT_FWD, 32, 0, 12) == 0
    assert ops.conv_igemm_form(7, 32, 0, 32) == 0 and ops.conv_wgrad_form(ops.CONVT_BWD, 32, 0, 32) == 0


def test_pool_restatement_is_pytorchs_maxpool():
    """Forward and the tie rule: an all-equal window sends the gradient to its first element, as PyTorch does."""
    import torch.nn.functional as F
    for i, shape in enumerate(UB.POOL):
        for kind in UB.POOL_DATA:
            x = UB.pool_data(kind, shape, torch.float32, i).double()
            xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
            y = F.max_pool2d(xt, 2)
            dy = UR.rnd(*y.shape, seed=i).double()
            (y * dy).sum().backward()
            ref, _ = UB.maxpool2(x)
            assert torch.equal(ref, y.detach().permute(0, 2, 3, 1)), (shape, kind)
            assert torch.equal(UB.maxpool2_bwd(x, dy.permute(0, 2, 3, 1)), xt.grad.permute(0, 2, 3, 1)), (shape, kind)


def test_act_restatements_are_pytorchs():
    import torch.nn.functional as F
    M, C, p = 37, 5, 0.5
    y, gamma, beta, rm, rv = UR.bn_case(M, C, torch.float32, seed=3, mean=0.3)
    keep = UB.keep_rows(M, C, p, 4)
    yt = y.double().clone().requires_grad_(True)
    gt = gamma.double().clone().requires_grad_(True)
    bt = beta.double().clone().requires_grad_(True)
    rm2, rv2 = rm.double().clone(), rv.double().clone()
    inv = 1.0 / (1.0 - UR.f32(p))
    out = F.leaky_relu(F.batch_norm(yt, rm2, rv2, gt, bt, True, UR.f32(0.1), UR.f32(1e-5)), 0.01) * keep.double() * inv
    r = UB.bn_act_train(y, gamma, beta, rm, rv, 0, UR.f32(0.1), UR.f32(1e-5), 0.01, p, keep)
    assert torch.allclose(r["out"][0], out.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(r["run_var"][0], rv2, rtol=1e-12) and torch.allclose(r["run_mean"][0], rm2, rtol=1e-12)
    dout = UR.rnd(M, C, seed=5).double()
    (out * dout).sum().backward()
    b = UB.bn_act_bwd(y, dout, r["scale"][0], r["shift"][0], r["mean"][0], r["invstd"][0], gamma, 0.01, p, keep)
    assert torch.allclose(b["dy"][0], yt.grad, rtol=1e-9, atol=1e-12)
    assert torch.allclose(b["dgamma"][0], gt.grad, rtol=1e-9, atol=1e-12) and torch.allclose(b["dbeta"][0], bt.grad, rtol=1e-9, atol=1e-12)
    # the gradient at z == 0 takes the slope
    z = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    F.leaky_relu(z, 0.01).sum().backward()
    assert z.grad.tolist() == [0.01] * 3
    ev, _ = UB.bn_act_eval(y, gamma, beta, rm, rv, UR.f32(1e-5), 0.01)
    assert torch.allclose(ev, F.leaky_relu(F.batch_norm(y.double(), rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.1, UR.f32(1e-5)), 0.01), rtol=1e-12, atol=1e-12)
    x, w, bias = UR.rnd(2, 3, 4, 6, seed=1), UR.rnd(5, 6, seed=2), UR.rnd(5, seed=3)
    ref, _ = UB.conv1x1(x, w, bias)
    assert torch.allclose(ref.permute(0, 3, 1, 2), F.conv2d(x.double().permute(0, 3, 1, 2), w.double()[:, :, None, None], bias.double()), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("argv, match", [(["--img_size", "40"], "not a multiple of 16")])
def test_entry_point_refuses_before_allocation(argv, match):
    from src.models.baselines import segmentation as S
    with pytest.raises(ValueError, match=match):
        S.main(argv + ["--synthetic", "--device", "cpu"])


def test_model_refusals_need_no_gpu():
    from src.third_party.unet import ConvBlock, UNet
    net = UNet(3, 2, init_channels=8)
    with pytest.raises(ValueError, match="multiple of 16"):
        net(torch.zeros(1, 3, 40, 40))
    with pytest.raises(ValueError, match="input channels"):
        net(torch.zeros(1, 2, 32, 32))
    masks = [torch.ones(1, 32 >> i, 32 >> i, 8 << i, dtype=torch.uint8) for i in range(5)]
    masks[2] = masks[2][:, :, :, :-1]
    with pytest.raises(ValueError, match=r"keep_masks\[2\]"):
        net(torch.zeros(1, 3, 32, 32), masks)
    with pytest.raises(ValueError, match="dropout_p"):
        ConvBlock(8, 8, 1.0)
