"""The cost of uia_resize_batch (reported in DESIGN.md §4 "Dataset folders") and what it takes off the loader workers.

  launch: ops.resize_batch on a ragged batch — `gray` B = 32, C = 1, 600 x 450 files with masks squashed to 224 x 224 (the supervised loaders), and `rgb`
          B = 256, C = 3, 500 x 375 files resampled to 298 x 224 with the centre 224 x 224 window (the contrastive loader's Resize + CenterCrop).  HIP
          events around one call (descriptor copy + kernel); the median of --reps calls after --warmup.  Beside each, PIL's time for the same batch on
          one host core (Image.resize per picture and mask, the median of three passes).
  loop:   (--loop) `loader_wait_ms` of the second epoch of the UNet segmentation baseline's training loop on a tree of --files 600 x 450 pictures read
          with --data_root, against the same pictures as a --data_pt file; each in a process of its own, at 8 and at 16 loader workers.

Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def speckle(H, W, C, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    fan = np.abs(xx - W / 2) < (yy + 3) * 0.8
    img = np.clip(rng.gamma(2.0, 0.18, (H, W, C)) * (0.55 + 0.45 * np.sin(np.hypot(yy, xx - W / 2) / 9.0))[..., None] * fan[..., None] * 255, 0, 255).astype(np.uint8)
    mask = ((((yy - H * 0.55) / (H * 0.22)) ** 2 + ((xx - W * 0.45) / (W * 0.3)) ** 2 <= 1) * 255).astype(np.uint8)
    return (img[..., 0] if C == 1 else img), mask


def time_launch(B, C, W, H, S, dst, corner, with_mask, args):
    from PIL import Image
    from src.datasets.folder import pack_ragged
    from uia_hip import ops
    dev = torch.device("cuda:0")
    dst_w, dst_h = dst
    pics = [speckle(H, W, C, 11 + b) for b in range(B)]
    buf, desc = pack_ragged([(px, mask if with_mask else None, (dst_h, dst_w, corner[1], corner[0])) for px, mask in pics])
    src, desc = buf.to(dev), desc.pin_memory()
    out_i = torch.empty(B, C, S, S, device=dev)
    out_m = torch.empty(B, 1, S, S, dtype=torch.uint8, device=dev) if with_mask else None
    ws = ops.resize_workspace(B, dev)
    fn = lambda: ops.resize_batch(src, desc, S, C, out_i, out_m, ws)
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    torch.set_num_threads(1)
    images = [(Image.fromarray(px, "L" if C == 1 else "RGB"), Image.fromarray(mask, "L").convert("1")) for px, mask in pics]
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        for im, mk in images:
            im.resize((dst_w, dst_h))
            if with_mask:
                mk.resize((dst_w, dst_h))
        host.append((time.perf_counter() - t0) * 1e3)
    # one picture of the batch against PIL, so that the figure is the figure of the right answer
    want = np.asarray(images[0][0].resize((dst_w, dst_h)))[corner[1]:corner[1] + S, corner[0]:corner[0] + S].reshape(S, S, C).transpose(2, 0, 1)
    same = bool(torch.equal(out_i[0].cpu(), torch.from_numpy(want.copy()).float() / 255))
    return {"ms": round(statistics.median(ms), 4), "min": round(ms[0], 4), "max": round(ms[-1], 4), "pil_one_core_ms": round(statistics.median(host), 2),
            "source_mb": round(buf.numel() / 1e6, 2), "equals_pil": same}


def write_tree(root, n, W, H, S):
    from PIL import Image
    for d in ("all/images", "all/masks", "segmentation/TIMING"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    names = [f"p{i:04d}.png" for i in range(n)]
    images, masks = [], []
    for i, name in enumerate(names):
        px, mask = speckle(H, W, 1, i)
        Image.fromarray(px, "L").save(os.path.join(root, "all/images", name))
        Image.fromarray(mask, "L").save(os.path.join(root, "all/masks", name))
        images.append(np.asarray(Image.fromarray(px, "L").resize((S, S))))
        masks.append(np.asarray(Image.fromarray(mask, "L").convert("1").resize((S, S)), dtype=np.uint8))
    a = n - 16
    for split, part in (("train", names[:a]), ("val", names[a:a + 8]), ("test", names[a + 8:])):
        with open(os.path.join(root, "segmentation/TIMING", f"{split}.txt"), "w") as f:
            f.write("\n".join(part) + "\n")
    torch.save({"images": torch.from_numpy(np.stack(images))[:, None], "labels": torch.from_numpy(np.stack(masks))[:, None], "names": names,
                "split": {"train": list(range(a)), "val": list(range(a, a + 8)), "test": list(range(a + 8, n))}}, os.path.join(root, "data.pt"))


def child(args):
    """One training run of the UNet baseline's loop with epoch timings; prints the second epoch's record."""
    import dataclasses
    from src.models import supervised
    from src.models.baselines import segmentation as entry
    source = ["--data_root", args.child] if args.source == "root" else ["--data_pt", os.path.join(args.child, "data.pt")]
    a = entry.get_args(source + ["--dataset", "TIMING", "--epochs", "2", "--val_every", "100", "--batch_size", "32", "--num_workers", str(args.num_workers), "--exp", "timing_" + args.source])
    a.train_snapshot_path = os.path.join(args.child, "runs_" + args.source)
    os.makedirs(a.train_snapshot_path, exist_ok=True)
    out = supervised.train(a, dataclasses.replace(supervised.SEGMENTATION, loop_timings=True), entry.prepare_model)
    print("EPOCH " + json.dumps(out["epochs"][1]))


def time_loop(args):
    res = {}
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, args.files, 600, 450, 224)
        for source, workers in (("root", 8), ("pt", 8), ("root", 16)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--source", source, "--num_workers", str(workers)],
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(r.stdout[-2000:] + r.stderr[-4000:])
            res[f"data_{source}_w{workers}"] = json.loads([line for line in r.stdout.splitlines() if line.startswith("EPOCH ")][-1][6:])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--files", type=int, default=272)
    ap.add_argument("--child", type=str, default=None)
    ap.add_argument("--source", type=str, default="root")
    ap.add_argument("--num_workers", type=int, default=8)
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = {"gray_b32_600x450_to_224": time_launch(32, 1, 600, 450, 224, (224, 224), (0, 0), True, args),
           "rgb_b256_500x375_to_298x224_window": time_launch(256, 3, 500, 375, 224, (298, 224), (37, 0), False, args)}
    if args.loop:
        out["unet_loop"] = time_loop(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
