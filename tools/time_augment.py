"""The augmentation stage's cost (reported in DESIGN.md §4 "Augmentation"): the uia_augment_batch launch by itself, and a training step of the UNet
baseline loop with the stage bypassed, on, and on with an all-empty program table.

  launch: ops.augment_batch on [B, 1, S, S] + uint8 masks at (B, S) = (32, 224) and (24, 518), for three tables: `drawn` (draw_programs with both flags
          on: about half the images untouched, six or seven ops in each of the others), `empty` (every program empty: the bit-for-bit copy) and `full` (13 ops in
          every image, every opcode among them, two crops).  HIP events around one call (table copy + kernel); the median of --reps calls after --warmup,
          five times over; the median of the five medians.
  step:   UNet(3, 2) in train mode, DiceCE, FlatAdapterOptimizer over all parameters, engine.segmentation_step on a resident [32, 1, 224, 224] batch — the
          loop body of src/models/supervised.train — with `bypass` (stage_for(...) is None: what --no-strong_augs --no-weak_augs and --synthetic
          run), `on` (BatchAugmenter with both flags) and `empty` (BatchAugmenter with no flag: it draws, copies and launches, every program empty).  HIP
          events around each step, nothing synchronised inside a round of --steps steps; the median step of a round, five rounds, the median and the spread
          (min .. max) of the five medians.  The stage adds no host synchronisation when `empty` lies within the spread of `bypass`.

Images are a speckled fan on black, 8-bit levels / 255 (what a --data_pt ultrasound file gives).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def fan_batch(B, S, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    r = np.hypot(yy + 2, xx - S / 2)
    fan = (np.abs(xx - S / 2) < (yy + 3) * 0.8) & (r < S * 1.02)
    img = np.clip(rng.gamma(2.0, 0.18, (B, S, S)) * (0.55 + 0.45 * np.sin(r / 9.0) * np.cos(xx / 15.0)) * fan * 255, 0, 255).astype(np.uint8)
    mask = (((yy - S * 0.55) / (S * 0.22)) ** 2 + ((xx - S * 0.45) / (S * 0.3)) ** 2 <= 1).astype(np.uint8)
    return torch.from_numpy(img.astype(np.float32) / np.float32(255))[:, None].contiguous(), torch.from_numpy(np.broadcast_to(mask, (B, S, S)).copy())[:, None].contiguous()


def full_table(B, S):
    from src.datasets import augment as A
    rows = [(A.CONTRAST, A.f32_bits(1.2), 0, 0), (A.AUTOCONTRAST, 0, 0, 0), (A.SHARPNESS, A.f32_bits(0.8), 0, 0), (A.POSTERIZE, 6, 0, 0), (A.BLUR, A.f32_bits(1.25), 0, 0),
            (A.BRIGHTNESS, A.f32_bits(0.9), 0, 0), (A.EQUALIZE, 0, 0, 0), (A.SOLARIZE, 200, 0, 0), (A.IDENTITY, 0, 0, 0), (A.CROP, 3, 1, S - S // 10), (A.HFLIP, 0, 0, 0),
            (A.CROP, 0, 2, S - 2), (A.VFLIP, 0, 0, 0)]
    t = np.zeros((B, A.ROWS, 4), dtype=np.int32)
    t[:, 0, 0], t[:, 0, 1] = len(rows), 1
    t[:, 1:1 + len(rows)] = rows
    return t


def median_of_medians(fn, warmup, reps, rounds=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    meds = []
    for _ in range(rounds):
        evs = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs.append((a, b))
        torch.cuda.synchronize()
        meds.append(statistics.median(a.elapsed_time(b) for a, b in evs))
    return {"ms": round(statistics.median(meds), 4), "min": round(min(meds), 4), "max": round(max(meds), 4)}


def time_launch(B, S, args):
    from src.datasets import augment as A
    from uia_hip import ops
    dev = torch.device("cuda:0")
    x, m = (t.to(dev) for t in fan_batch(B, S, S))
    out_i, out_m, ws = torch.empty_like(x), torch.empty_like(m), ops.augment_workspace(B, S, dev)
    drawn = A.draw_programs(B, S, True, True, True, A.make_rng(1))
    res = {"ops_drawn": int(drawn[:, 0, 0].sum()), "images_touched": int((drawn[:, 0, 0] > 0).sum())}
    for name, t in (("drawn", drawn), ("empty", np.zeros_like(drawn)), ("full", full_table(B, S))):
        table = torch.from_numpy(t).pin_memory()
        res[name] = median_of_medians(lambda: ops.augment_batch(x, m, table, out_i, out_m, ws), args.warmup, args.reps)
    return res


def time_step(args):
    from src.datasets import augment as A
    from src.datasets.segmentation import as_model_input
    from src.losses.dice import DiceCELoss
    from src.third_party.unet import UNet
    from uia_hip import functional as UF
    from uia_hip.engine import FlatAdapterOptimizer, segmentation_step
    dev = torch.device("cuda:0")
    B, S = 32, 224
    UF.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(1)
    model = UNet(in_channels=3, num_classes=2).to(dev).train()
    opt = FlatAdapterOptimizer([(n, p) for n, p in model.named_parameters() if p.requires_grad], lr=1e-4, betas=(0.9, 0.95), weight_decay=0.01, max_norm=0.0)
    criterion = DiceCELoss(smooth_nr=1e-8, smooth_dr=1e-8)
    x, m = (t.to(dev) for t in fan_batch(B, S, 7))
    stages = {"bypass": None, "on": A.BatchAugmenter(True, True, True, seed=1), "empty": A.BatchAugmenter(False, False, True, seed=1), "bypass_again": None}
    res = {}
    for name, stage in stages.items():
        bufs = {}

        def step():
            images, labels = (x, m) if stage is None else stage(x, m)
            images, labels = as_model_input(images, labels, 3, bufs, widen=False)
            segmentation_step(model, criterion, opt, images, labels, lr=1e-4)

        res[name] = median_of_medians(step, args.warmup, args.steps)
        if stage is not None:
            res[name]["augmented_images"] = stage.augmented
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no_step", action="store_true")
    args = ap.parse_args()
    out = {"launch_b32_s224": time_launch(32, 224, args), "launch_b24_s518": time_launch(24, 518, args)}
    if not args.no_step:
        out["unet_step_b32_s224"] = time_step(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
