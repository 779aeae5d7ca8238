"""Times the few-shot training path against the loader path on the same data: milliseconds per epoch of

  resident   python -m src.models.biomedclip.fewshot_segmentation --train_ratio 1.0   (the training rows live on the device, one launch forms a batch)
  loader     python -m src.models.biomedclip.segmentation                              (loader workers, shared-memory ring, per-batch copy, the stage's launch)

on a `--data_pt` file this tool writes itself: N = 8 and N = 64 training rows of 224 x 224 uint8 with masks (4 validation and 4 test rows), the default
BiomedCLIP geometry from random weights, bf16, augmentation on, batch 32, 30 epochs with one validation at the very end (outside the epoch records).
The few-shot loader contract gives B = min(32, N); the loader entry drops ragged batches, so at N = 8 it runs with --batch_size 8: the same N and the
same batch size on both sides.  Every run is a fresh process; the two paths alternate, RUNS times each, in one call.  A run's figure is the median
of its `epochs` records (--stats_json) behind the first WARM epochs; printed per run, then as a range over the runs.

    python tools/time_fewshot.py [--runs 5] [--epochs 30] [--sizes 8,64] [--out DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nextgen-uia_amd")
WARM = 5
RUN_LIMIT_S = 300


def write_blob(path, n, S=224, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    total = n + 8
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    cx = torch.randint(S // 4, 3 * S // 4, (total,), generator=g)
    labels = (((yy[None] - S // 2) ** 2 + (xx[None] - cx[:, None, None]) ** 2) <= (S // 5) ** 2)[:, None].to(torch.uint8) * 255
    images = (torch.randint(0, 120, (total, 1, S, S), generator=g) + labels // 2).to(torch.uint8)
    torch.save({"images": images, "labels": labels,
                "split": {"train": list(range(n)), "val": list(range(n, n + 4)), "test": list(range(n + 4, n + 8))}}, path)


def one_run(module, extra, blob, n, epochs, work):
    stats = os.path.join(work, "stats.json")
    if os.path.exists(stats):
        os.remove(stats)
    cmd = [sys.executable, "-m", module, "--data_pt", blob, "--batch_size", str(min(32, n)), "--epochs", str(epochs), "--val_every", str(10 * epochs),
           "--no-viz", "--stats_json", stats, "--exp", "time_fewshot", "--dataset", f"N{n}"] + extra
    r = subprocess.run(cmd, cwd=work, env=dict(os.environ, PYTHONPATH=PKG), capture_output=True, text=True, timeout=RUN_LIMIT_S)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    out = json.load(open(stats))
    ms = [e["ms"] for e in out["epochs"]]
    assert len(ms) == epochs and all(e["updates"] == n // min(32, n) for e in out["epochs"]), out["epochs"][:3]
    return statistics.median(ms[WARM:]), out


def main(argv=None):
    p = argparse.ArgumentParser(__doc__.splitlines()[0])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--epochs", type=int, default=30)
    p.add_argument("--sizes", type=str, default="8,64")
    p.add_argument("--out", type=str, default=None, help="folder for time_fewshot.json")
    a = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_fewshot needs the GPU: an epoch time taken anywhere else says nothing")
    report = {}
    with tempfile.TemporaryDirectory() as work:
        for n in (int(v) for v in a.sizes.split(",")):
            blob = os.path.join(work, f"fewshot_{n}.pt")
            write_blob(blob, n)
            paths = {"resident": ("src.models.biomedclip.fewshot_segmentation", ["--train_ratio", "1.0"]), "loader": ("src.models.biomedclip.segmentation", [])}
            got = {k: [] for k in paths}
            for r in range(a.runs):
                for name, (module, extra) in paths.items():          # alternating
                    ms, out = one_run(module, extra, blob, n, a.epochs, work)
                    got[name].append(ms)
                    print(f"N={n} run {r} {name:8s} {ms:8.2f} ms / epoch ({out['epochs'][0]['updates']} updates, {out['augmented_images']} augmented images)", flush=True)
            report[n] = got
            for name, v in got.items():
                print(f"N={n} {name:8s} {min(v):.2f} .. {max(v):.2f} ms / epoch (median {statistics.median(v):.2f}) over {len(v)} runs", flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "time_fewshot.json"), "w") as f:
            json.dump(report, f, indent=1)
    return report


if __name__ == "__main__":
    main()
