"""Writes the DINOv2 segmentation-decoder fixtures under tests/golden/ from the imported reference (its own modules, run on the CPU in float64):

    reference_dino_seg_cli_table.json   the argparse table of src/models/dino/segmentation.py (flag -> default / action / choices, as source text)
    dino_seg_keys.json    the state-dict names and shapes of setup_decoders(768, [1e-4], 2, "unet", 518, 14)[0] (AllDecoders, BatchNorm buffers
                          included) and its ModuleDict key
    dino_seg_small.npz    on the small geometry of tests/unet_reference.SMALL, with the seeded weights and inputs of that module: the train-mode
                          logits, the BatchNorm buffers after that forward, every parameter's gradient for the seeded upstream gradient, and the
                          eval-mode logits that follow

Only names and recorded outputs are stored, never source text; weights and inputs are regenerated from seeds by the tests.  dinov2.py imports
torchvision.transforms, which the build does not carry: a stub stands in for it whose transforms.Resize(size, BICUBIC) calls exactly what
torchvision 0.24's Resize runs on a float tensor, F.interpolate(x, size, mode="bicubic", align_corners=False, antialias=True).

    python tools/gen_dino_seg_golden.py REFERENCE_DIR
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.gen_host_fixtures import argparse_table  # noqa: E402

import unet_reference as UR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def import_reference(reference_dir):
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    trt = types.ModuleType("torchvision.transforms.transforms")

    class InterpolationMode:
        BICUBIC = "bicubic"

    class Resize:
        def __init__(self, size, interpolation=InterpolationMode.BICUBIC):
            assert interpolation == InterpolationMode.BICUBIC
            self.size = tuple(size)

        def __call__(self, x):
            return UR.resize(x, self.size)

    trt.Resize, trt.InterpolationMode = Resize, InterpolationMode
    tr.transforms = trt
    tv.transforms = tr
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.transforms": trt})
    sys.path.insert(0, reference_dir)
    from src.third_party.dino import dinov2
    return dinov2


def main(reference_dir):
    dinov2 = import_reference(reference_dir)
    table = argparse_table(os.path.join(reference_dir, "src/models/dino/segmentation.py"))
    with open(os.path.join(GOLDEN, "reference_dino_seg_cli_table.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    cuda = nn.Module.cuda
    nn.Module.cuda = lambda self, device=None: self          # setup_decoders calls .cuda(); the names do not depend on the device
    try:
        decoders, _ = dinov2.setup_decoders(768, [1e-4], num_classes=2, decoder_type="unet", image_size=518, patch_size=14)
    finally:
        nn.Module.cuda = cuda
    keys = {"module_keys": list(decoders.decoders_dict.keys()), "state": [[k, list(v.shape)] for k, v in decoders.state_dict().items()]}
    with open(os.path.join(GOLDEN, "dino_seg_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")

    S = UR.SMALL
    P = UR.seeded_state(S["embed_dim"], S["num_classes"], S["seed"])
    maps, dlogits = UR.seeded_inputs(**S)
    dec = dinov2.UNetDecoder(S["embed_dim"], S["num_classes"], image_size=S["image_size"], resize_image=True, patch_size=S["patch_size"]).double()
    assert [(k, tuple(v.shape)) for k, v in dec.state_dict().items()] == [(k, tuple(s)) for k, s in UR.state_shapes(S["embed_dim"], S["num_classes"])]
    dec.load_state_dict(P)
    dec.train()
    out = dec([(m, None) for m in maps])
    (out * dlogits).sum().backward()
    rec = {"train_out": out.detach().float().numpy()}
    for k, v in dec.state_dict().items():
        if "running" in k or "num_batches" in k:
            rec["buf:" + k] = v.numpy() if v.dtype == torch.int64 else v.float().numpy()
    for k, p in dec.named_parameters():
        rec["grad:" + k] = p.grad.float().numpy()
    dec.eval()
    with torch.no_grad():
        rec["eval_out"] = dec([(m, None) for m in maps]).float().numpy()
    np.savez_compressed(os.path.join(GOLDEN, "dino_seg_small.npz"), **rec)
    print("wrote", len(rec), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/gen_dino_seg_golden.py REFERENCE_DIR")
    main(sys.argv[1])
