"""Writes the UNet-baseline fixtures under tests/golden/ from the imported reference (its own modules, run on the CPU in float64):

    reference_baseline_seg_cli_table.json   the argparse table of src/models/baselines/segmentation.py (flag -> default / action / choices, as source text)
    unet_baseline_keys.json       the state-dict names and shapes of UNet(3, 2) (BatchNorm buffers included)
    unet_baseline_small.npz       on the small geometry of tests/unet_baseline_reference.SMALL (UNet(3, 2, init_channels=8), B = 2, 32x32), with the
                                  seeded weights, inputs and keep masks of that module: the train-mode logits, the BatchNorm buffers after that
                                  forward, every parameter's gradient for the seeded upstream gradient, and the eval-mode logits that follow
    unet_baseline_small_down4.npz the gradients of encoder.down4 (885 kB of the 1.9 MB), apart so that no file passes 1 MiB

Each nn.Dropout of the reference is replaced at generation time by x·keep/(1−p) with the seeded keep mask.  Only names and recorded values are
stored, never source text; weights, inputs and masks are regenerated from seeds by the tests.

    python tools/gen_unet_baseline_golden.py REFERENCE_DIR
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.gen_host_fixtures import argparse_table  # noqa: E402

import unet_baseline_reference as UB  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
APART = "grad:encoder.down4."


class MaskDrop(nn.Module):
    def __init__(self, keep, p):
        super().__init__()
        self.keep, self.p = keep, p

    def forward(self, x):
        return x * self.keep / (1 - self.p) if self.training else x


def main(reference_dir):
    sys.path.insert(0, reference_dir)
    from src.third_party.unet import UNet
    table = argparse_table(os.path.join(reference_dir, "src/models/baselines/segmentation.py"))
    with open(os.path.join(GOLDEN, "reference_baseline_seg_cli_table.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    keys = {"state": [[k, list(v.shape)] for k, v in UNet(3, 2).state_dict().items()]}
    with open(os.path.join(GOLDEN, "unet_baseline_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")

    S = UB.SMALL
    P = UB.seeded_state(S["in_channels"], S["num_classes"], S["init_channels"], S["seed"])
    x, dlogits = UB.seeded_inputs(**S)
    masks = UB.seeded_masks(**S)
    net = UNet(S["in_channels"], S["num_classes"], init_channels=S["init_channels"]).double()
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(s)) for k, s in UB.state_shapes(S["in_channels"], S["num_classes"], S["init_channels"])]
    net.load_state_dict(P)
    enc = net.encoder
    blocks = [enc.in_conv, enc.down1.maxpool_conv[1], enc.down2.maxpool_conv[1], enc.down3.maxpool_conv[1], enc.down4.maxpool_conv[1]]
    for blk, keep, p in zip(blocks, masks, UB.DROPOUT):
        assert isinstance(blk.conv_conv[3], nn.Dropout) and blk.conv_conv[3].p == p
        blk.conv_conv[3] = MaskDrop(keep, p)
    for m in net.modules():
        assert not isinstance(m, nn.Dropout) or m.p == 0.0
    net.train()
    out = net(x)
    (out * dlogits).sum().backward()
    rec = {"train_out": out.detach().float().numpy()}
    for k, v in net.state_dict().items():
        if UB.is_buffer(k):
            rec["buf:" + k] = v.numpy() if v.dtype == torch.int64 else v.float().numpy()
    for k, p in net.named_parameters():
        rec["grad:" + k] = p.grad.float().numpy()
    net.eval()
    with torch.no_grad():
        rec["eval_out"] = net(x).float().numpy()
    np.savez_compressed(os.path.join(GOLDEN, "unet_baseline_small.npz"), **{k: v for k, v in rec.items() if not k.startswith(APART)})
    np.savez_compressed(os.path.join(GOLDEN, "unet_baseline_small_down4.npz"), **{k: v for k, v in rec.items() if k.startswith(APART)})
    print("wrote", len(rec), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/gen_unet_baseline_golden.py REFERENCE_DIR")
    main(sys.argv[1])
