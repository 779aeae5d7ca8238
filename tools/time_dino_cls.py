"""Times the DINOv2 classification path on one GPU: the long attention forward (uia_attn_fwd_long) at B = 24, H = 12, L = 1370 on random data with torch's
SDPA on the same shape as a yardstick, the frozen ViT-B/14 tower at 518 px (features of a batch) and one training step of the entry point
(tower + head + focal loss + backward + AdamW).  One JSON line per figure.

    python tools/time_dino_cls.py [--batch 24] [--reps 20]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "nextgen-uia_amd"))


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from uia_hip import ops
    from uia_hip import functional as UF
    from uia_hip.engine import FlatAdapterOptimizer, segmentation_step
    from src.losses.focal import FocalLoss
    from src.models.dino.classification import build_model

    B, H, L = a.batch, 12, 1370
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B * L, 3 * H * 64, device="cuda", generator=g).to(torch.bfloat16)
    out = torch.empty(B * L, H * 64, device="cuda", dtype=torch.bfloat16)
    D = H * 64
    flop = 4.0 * B * H * L * L * 64
    med, best = timed(lambda: ops.attn_fwd_long(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, B, H, L), a.reps)
    print(json.dumps({"what": "attn_fwd_long bf16", "B": B, "H": H, "L": L, "us": round(med * 1e3, 1), "best_us": round(best * 1e3, 1), "tflops": round(flop / med / 1e9, 1)}))
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(B, L, H, 64).transpose(1, 2).contiguous() for i in range(3))
    sdpa = torch.nn.functional.scaled_dot_product_attention
    med, best = timed(lambda: sdpa(q, k, v), a.reps)
    print(json.dumps({"what": "torch SDPA bf16 (yardstick)", "B": B, "H": H, "L": L, "us": round(med * 1e3, 1), "best_us": round(best * 1e3, 1), "tflops": round(flop / med / 1e9, 1)}))
    del qkv, out, q, k, v

    UF.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model(518, 14, 2).cuda()
    model.train()
    images = torch.rand(B, 1, 518, 518, device="cuda")
    labels = torch.arange(B, device="cuda") % 2
    with torch.no_grad():
        med, best = timed(lambda: model.feature_model(images), max(5, a.reps // 2))
    print(json.dumps({"what": "frozen ViT-B/14 tower at 518 px", "batch": B, "ms": round(med, 2), "best_ms": round(best, 2)}))
    opt = FlatAdapterOptimizer([(n, p) for n, p in model.named_parameters() if p.requires_grad], lr=1e-4, betas=(0.9, 0.95), weight_decay=0.01, max_norm=0.0)
    crit = FocalLoss(to_onehot_y=True)
    med, best = timed(lambda: segmentation_step(model, crit, opt, images, labels, lr=1e-4), max(5, a.reps // 2))
    print(json.dumps({"what": "training step (tower + head + focal + AdamW)", "batch": B, "ms": round(med, 2), "best_ms": round(best, 2)}))


if __name__ == "__main__":
    main()
