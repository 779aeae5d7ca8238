"""HD95 / ASD kernel timing (uia_surface_distances, csrc/surface.hip) and its share of a CLIPSeg validation pass (reported in DESIGN.md §4).

  * ops.surface_distances at B = 128, 224 x 224: realistic blob masks (an ellipse label as bench.py's synthetic batch draws it, the prediction the same
    ellipse shifted and resized) and iid-noise logits against the same labels (the worst case for edge count);
  * B = 16 at 1024 x 1024, iid-noise logits;
  * one CLIPSeg BUSI validation batch at bs 128 (bench.py --config clipseg's model and flags, bf16): forward, forward + MetricAccumulator.update without
    the surface metrics, forward + update with them.
Every figure is the median of HIP-event times over --reps calls after --warmup calls.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd")]
import torch  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4)


def blob_pair(B, S, seed, dev):
    """labels: bench.py's synthetic ellipses; prediction logits: each ellipse shifted by up to 6 px and scaled by 0.85-1.15, random logit margins."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    c = torch.rand(B, 2, generator=g) * S * 0.5 + S * 0.25
    r = torch.rand(B, 2, generator=g) * S * 0.2 + S * 0.08
    ell = lambda c_, r_: ((yy[None] - c_[:, 0, None, None]) / r_[:, 0, None, None]) ** 2 + ((xx[None] - c_[:, 1, None, None]) / r_[:, 1, None, None]) ** 2 <= 1
    label = ell(c, r)[:, None].float()
    pred = ell(c + (torch.rand(B, 2, generator=g) - 0.5) * 12, r * (0.85 + 0.3 * torch.rand(B, 2, generator=g)))
    l0 = torch.randn(B, S, S, generator=g)
    l1 = torch.where(pred, l0 + 0.5, l0 - 0.5)
    return torch.stack([l0, l1], 1).to(dev), label.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-clipseg", action="store_true")
    args = ap.parse_args()
    from uia_hip import ops
    dev = torch.device("cuda:0")
    out = {}
    logits, label = blob_pair(128, 224, 0, dev)
    out["blobs_b128_224_ms"] = timed(lambda: ops.surface_distances(logits, label), args.warmup, args.reps)
    noise = torch.randn(128, 2, 224, 224, generator=torch.Generator().manual_seed(1)).to(dev)
    out["noise_b128_224_ms"] = timed(lambda: ops.surface_distances(noise, label), args.warmup, args.reps)
    _, label_big = blob_pair(16, 1024, 2, dev)
    noise_big = torch.randn(16, 2, 1024, 1024, generator=torch.Generator().manual_seed(3)).to(dev)
    out["noise_b16_1024_ms"] = timed(lambda: ops.surface_distances(noise_big, label_big), 2, max(3, args.reps // 4))
    del noise_big, label_big
    if not args.no_clipseg:
        from src.models.clipseg import segmentation as S
        from src.utils.tools import MetricAccumulator
        from uia_hip import functional as UF
        UF.set_compute_dtype(torch.bfloat16)
        sargs = S.get_args(["--synthetic", "--batch_size", "128"])
        sargs.device = str(dev)
        torch.manual_seed(0)
        model = S.prepare_model(sargs)
        model.eval()
        images, labels = S.synthetic_batch(128, 224, 1, str(dev))
        sargs.dataset = "BUSI"
        prompt = S.get_prompt(sargs).to(dev).repeat(128, 1)
        with_surf = MetricAccumulator(type="seg", criterion=S.criterion, num_classes=2)
        without = MetricAccumulator(type="seg", criterion=S.criterion, num_classes=2)
        without.num_classes = 0                                  # the same update() without the surface-distance call

        def val(acc):
            with torch.no_grad():
                preds = model(images, input_ids=prompt)
                if acc is not None:
                    acc.update(preds, labels)
                    if len(acc._dice) > 64:
                        acc.reset()
        out["clipseg_val_forward_ms"] = timed(lambda: val(None), args.warmup, args.reps)
        out["clipseg_val_forward_update_no_surface_ms"] = timed(lambda: val(without), args.warmup, args.reps)
        out["clipseg_val_forward_update_ms"] = timed(lambda: val(with_surf), args.warmup, args.reps)
        with torch.no_grad():
            preds = model(images, input_ids=prompt)
        out["clipseg_preds_surface_ms"] = timed(lambda: ops.surface_distances(preds, labels), args.warmup, args.reps)
        out["blobs_frac_of_val_forward"] = round(out["blobs_b128_224_ms"] / out["clipseg_val_forward_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
