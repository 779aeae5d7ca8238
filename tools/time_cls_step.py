"""One supervised classification step at the reference defaults (BiomedCLIP ViT-B/16, batch 32, 224 x 224, bf16, TimmCLIPAdapter(task="cls") on layers
3/6/9): engine.segmentation_step with FocalLoss(to_onehot_y=True), as src/models/biomedclip/classification.py runs it.  Two configurations: the baseline
(no adapters in the backbone, script step 3.1) and Mona `hybrid` loaded from a fine-tune checkpoint (step 3.2; random adapter weights here).  Reported in
DESIGN.md; no target.

    python tools/time_cls_step.py [--steps 20] [--warmup 5]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd")]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from src.adapters import inject_mona_variant_to_open_clip
    from src.datasets.classification import synthetic_split
    from src.models.biomedclip import classification as cli
    from src.third_party.biomedclip.model import create_biomedclip
    from uia_hip import functional as UF
    from uia_hip.engine import FlatAdapterOptimizer, segmentation_step
    UF.set_compute_dtype(torch.bfloat16)
    images, labels = synthetic_split(32, 224, 1)
    images, labels = images.cuda(), labels.cuda()
    with tempfile.TemporaryDirectory() as tmp:
        m = create_biomedclip(seed=1)
        inject_mona_variant_to_open_clip(m, variant="hybrid", bottleneck_dim=64)
        ck = os.path.join(tmp, "mona.pth")
        torch.save({k: v for k, v in m.state_dict().items() if "mona" in k}, ck)
        del m
        for name, extra in (("baseline", []), ("mona hybrid", ["--mona_weights", ck])):
            args = cli.get_args(["--device", "cuda:0"] + extra)
            model = cli.prepare_model(args)
            model.train()
            opt = FlatAdapterOptimizer([(n, p) for n, p in model.named_parameters() if p.requires_grad], lr=1e-4, betas=(0.9, 0.95), weight_decay=0.01,
                                       max_norm=0.0)
            for _ in range(a.warmup):
                loss, _ = segmentation_step(model, cli.criterion, opt, images, labels, lr=1e-4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss, _ = segmentation_step(model, cli.criterion, opt, images, labels, lr=1e-4)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.steps
            n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
            print(f"classification step, BiomedCLIP ViT-B/16 bs=32 bf16, {name}: {dt * 1e3:.2f} ms/step, {32 / dt:.0f} images/s, "
                  f"loss {float(loss):.4f}, trainable {n_train}")
            del model, opt


if __name__ == "__main__":
    main()
