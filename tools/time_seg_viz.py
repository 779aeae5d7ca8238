"""Timing of the segmentation pictures (reported in DESIGN.md §4 "Segmentation visualisation").

  * uia_seg_viz alone, HIP events: the median of --reps launches after --warmup, --rounds times over, with the spread of the medians.  B = 32, S = 224 (the
    four-pixels-per-thread kernel) and B = 24, S = 518 (the pixel-per-thread kernel), fp32 and uint8 labels, one-channel images; then B = 32 and B = 128 at
    S = 224 on both kernels (the outputs one byte into their buffers take the pixel-per-thread one); bytes moved per second
    (what the kernel has to read and write, from the shapes) against the part's HBM rate (8.0 TB/s spec, 6.29 TB/s measured float4 copy).
  * --loop: wall time of test() of `baselines/segmentation.py --synthetic --synthetic_test N` with --viz and with --no-viz, alternating --loop_reps times in
    this process (the checkpoint is a randomly initialised UNet saved once), the writers' per-file encode time and the file sizes, at each --levels value.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd")]
import torch  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def kernel_times(B, S, label_dtype, warmup, reps, rounds, shift=0):
    """shift = 1: every output starts one byte into its buffer, which sends an aligned size to the pixel-per-thread kernel."""
    from uia_hip import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(S)
    logits = torch.randn(B, 2, S, S, generator=g).to(dev)
    images = torch.rand(B, 1, S, S, generator=g).to(dev)
    labels = (torch.rand(B, 1, S, S, generator=g) < 0.3).to(label_dtype).to(dev)
    outs = [torch.empty(B * S * S * c + shift, dtype=torch.uint8, device=dev)[shift:].view((B, S, S, 3) if c == 3 else (B, S, S)) for c in (3, 3, 1)]
    form = ops.seg_viz_form(logits, images, labels, *outs)
    medians = []
    for _ in range(rounds):
        for _ in range(warmup):
            ops.seg_viz(logits, images, labels, *outs)
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.seg_viz(logits, images, labels, *outs)
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        medians.append(statistics.median(us))
    moved = B * S * S * (12 + labels.element_size() + 7)        # image + two logit planes + label in, 3 + 3 + 1 bytes out
    mid = statistics.median(medians)
    return {"B": B, "S": S, "labels": str(label_dtype).replace("torch.", ""), "kernel": "quad" if form else "pixel", "us_median": round(mid, 2),
            "us_min": round(min(medians), 2), "us_max": round(max(medians), 2), "bytes": moved, "TB_per_s": round(moved / mid * 1e-6, 3),
            "of_hbm_spec": round(moved / (mid * 1e-6) / HBM_SPEC, 3), "of_hbm_copy": round(moved / (mid * 1e-6) / HBM_COPY, 3)}


def loop_times(n_test, batch, img, levels, reps):
    from src.models import supervised
    from src.models.baselines import segmentation as cli
    from src.utils import viz
    out = {"n_test": n_test, "batch_size": batch, "img_size": img, "levels": {}}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            argv = ["--synthetic", "--synthetic_test", str(n_test), "--batch_size", str(batch), "--img_size", str(img), "--num_workers", "0", "--exp", "t"]
            args = cli.get_args(argv)
            os.makedirs("runs/t/LN-INT/train")
            torch.save(cli.prepare_model(args).state_dict(), "runs/t/LN-INT/train/best_model.pth")

            def one(flag):
                a = cli.get_args(argv + ["--test", flag])
                a.train_snapshot_path, a.test_snapshot_path = "runs/t/LN-INT/train", "runs/t/LN-INT/test"
                os.makedirs(a.test_snapshot_path, exist_ok=True)
                supervised.setup_logging(a, a.test_snapshot_path)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stats = supervised.test(a, supervised.SEGMENTATION, cli.prepare_model)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, stats

            one("--no-viz")                                     # code objects, the first prefetcher
            for level in levels:
                viz.PNG_LEVEL = level
                seen = []
                real = viz.SegVisualizer.close

                def close(self, _real=real, _seen=seen):
                    _real(self)
                    _seen.append((self.files, self.bytes, self.encode_s))
                viz.SegVisualizer.close = close
                orig_init = viz.SegVisualizer.__init__

                def init(self, *a, _orig=orig_init, _level=level, **k):
                    k.setdefault("level", _level)
                    _orig(self, *a, **k)
                viz.SegVisualizer.__init__ = init
                try:
                    with_viz, without = [], []
                    for _ in range(reps):
                        without.append(one("--no-viz")[0])
                        with_viz.append(one("--viz")[0])
                finally:
                    viz.SegVisualizer.close, viz.SegVisualizer.__init__ = real, orig_init
                files, size, enc = seen[-1]
                out["levels"][str(level)] = {"test_s_no_viz": [round(v, 3) for v in without], "test_s_viz": [round(v, 3) for v in with_viz], "files": files,
                                             "bytes_per_image": round(3 * size / files), "encode_ms_per_file": round(1e3 * enc / files, 3)}
        finally:
            os.chdir(cwd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--loop_test", type=int, default=256)
    ap.add_argument("--loop_reps", type=int, default=3)
    ap.add_argument("--levels", type=str, default="1,6")
    args = ap.parse_args()
    out = {"kernel": [kernel_times(B, S, dt, args.warmup, args.reps, args.rounds) for B, S in ((32, 224), (24, 518)) for dt in (torch.float32, torch.uint8)]}
    out["kernel"].append(kernel_times(32, 224, torch.float32, args.warmup, args.reps, args.rounds, shift=1))
    out["kernel"].append(kernel_times(128, 224, torch.float32, args.warmup, args.reps, args.rounds))           # about the bytes of the S = 518 batch, aligned
    out["kernel"].append(kernel_times(128, 224, torch.float32, args.warmup, args.reps, args.rounds, shift=1))
    if args.loop:
        out["loop"] = loop_times(args.loop_test, 32, 224, [int(v) for v in args.levels.split(",")], args.loop_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
