"""Writes the DINOv2 fixtures under tests/golden/ from the imported reference (its own modules, run on the CPU in float64):

    reference_dino_cli_tables.json   the argparse table of src/models/dino/classification.py (flag -> default / action / choices, as source text)
    dino_vitb14_keys.json            the state-dict names and shapes of DINOV2Encoder(vit_base(img_size=518, patch_size=14)) and ClassificationHead(768, 2, 4)
    dino_small.npz                   features [B, 5·D] and logits of the reference's DINOV2Encoder + ClassificationHead(layers=4) on the small
                                     geometry of tests/dino_reference.SMALL, with the seeded weights and images of that module

Only tables, names and recorded outputs are stored, never source text.  dinov2.py imports torchvision.transforms, which the build does not carry:
a stub module stands in for it (nothing of it is used by the classes read here).

    python tools/gen_dino_golden.py REFERENCE_DIR
"""
import json
import os
import sys
import types
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.gen_host_fixtures import argparse_table  # noqa: E402
import dino_reference as DR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def import_reference(reference_dir):
    if "torchvision" not in sys.modules:
        tv = types.ModuleType("torchvision")
        tr = types.ModuleType("torchvision.transforms")
        tr.transforms = types.ModuleType("torchvision.transforms.transforms")
        tv.transforms = tr
        sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.transforms": tr.transforms})
    sys.path.insert(0, reference_dir)
    from src.third_party.dino import dinov2, vision_transformer
    from src.third_party.dino.layers import MemEffAttention, NestedTensorBlock
    return vision_transformer, dinov2, partial(NestedTensorBlock, attn_class=MemEffAttention)


def main(reference_dir):
    vit, dinov2, block_fn = import_reference(reference_dir)
    table = argparse_table(os.path.join(reference_dir, "src/models/dino/classification.py"))
    with open(os.path.join(GOLDEN, "reference_dino_cli_tables.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")

    enc = dinov2.DINOV2Encoder(vit.vit_base(img_size=518, patch_size=14), n_last_blocks=4)
    head = dinov2.ClassificationHead(embed_dim=768, num_classes=2, layers=4)
    keys = {"encoder": [[k, list(v.shape)] for k, v in enc.state_dict().items()], "classifier": [[k, list(v.shape)] for k, v in head.state_dict().items()],
            "ls_identity": type(enc.encoder.blocks[0][0].ls1).__name__}
    with open(os.path.join(GOLDEN, "dino_vitb14_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")

    S = DR.SMALL
    torch.manual_seed(0)
    model = vit.DinoVisionTransformer(img_size=S["img_size"], patch_size=S["patch_size"], embed_dim=S["embed_dim"], depth=S["depth"],
                                      num_heads=S["num_heads"], mlp_ratio=4, block_fn=block_fn)
    enc = dinov2.DINOV2Encoder(model, n_last_blocks=4)
    head = dinov2.ClassificationHead(embed_dim=S["embed_dim"], num_classes=S["num_classes"], layers=4)
    state = DR.seeded_state(S["img_size"], S["patch_size"], S["embed_dim"], S["depth"], S["num_classes"], S["seed"])
    enc.load_state_dict({k: v for k, v in state.items() if k.startswith("encoder.")}, strict=True)
    head.load_state_dict({k: v for k, v in state.items() if k.startswith("linear.")}, strict=True)
    enc.double().eval()
    head.double()
    images = DR.seeded_images(S["batch"], S["img_size"], S["seed"])
    with torch.no_grad():
        feats_list = enc(images.double())
        logits = head(feats_list)
        feats = torch.cat([feats_list[0][1], feats_list[1][1], feats_list[2][1], feats_list[3][1], feats_list[3][0].mean(dim=1)], dim=1)
    np.savez_compressed(os.path.join(GOLDEN, "dino_small.npz"), features=feats.numpy(), logits=logits.numpy())
    f64, l64 = DR.forward(images, state, S["num_heads"], S["patch_size"])
    print(f"wrote reference_dino_cli_tables.json ({len(table)} flags), dino_vitb14_keys.json ({len(keys['encoder'])} + {len(keys['classifier'])} names), "
          f"dino_small.npz; restatement vs reference: features {float((f64 - feats).abs().max()):.2e}, logits {float((l64 - logits).abs().max()):.2e}")


if __name__ == "__main__":
    main(sys.argv[1])
