"""The cost of the --finetune_root path (reported in DESIGN.md §4 "Caption folders"), with tools/time_resize.py's method.

  launch: ops.resize_batch_rgb on B = 256 pictures of 500 x 375 resampled to 298 x 224 with the centre 224 x 224 window — all RGB, and every second
          one gray — beside ops.resize_batch (C = 3) on the same all-RGB batch in the same run.  HIP events around one call (descriptor copy + kernel);
          the median of --reps calls after --warmup.
  loop:   (--loop) the BiomedCLIP fine-tune CLI's second epoch — `ms`, `loader_wait_ms`, pictures per second — on a generated tree of --files JPEG
          files (500 x 375, every fourth gray) read with --finetune_root, against the same pictures as a --data_pt file; each a process of its own.
          Beside them the time one host core takes to decode one file, and to decode + Resize + CenterCrop it as the reference's worker does.

Prints one JSON line."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_resize import speckle  # noqa: E402

W, H, S = 500, 375, 224
WORDS = "axial ct scan of the liver shows a hypodense lesion with irregular margins and mild enhancement in the portal venous phase".split()


def time_launches(args):
    from src.datasets.captions import geometry
    from src.datasets.folder import pack_ragged
    from uia_hip import ops
    dev = torch.device("cuda:0")
    B, geom = 256, geometry(W, H, S)
    pics = [speckle(H, W, 3, 11 + b)[0] for b in range(B)]
    out = torch.empty(B, 3, S, S, device=dev)
    ws = ops.resize_workspace(B, dev)

    def timed(fn):
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
        return {"ms": round(statistics.median(ms), 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}

    res = {}
    for name, gray_every in (("all_rgb", 0), ("half_gray", 2)):
        items = [(px[..., 1].copy() if gray_every and b % gray_every else px, None, geom) for b, px in enumerate(pics)]
        buf, desc = pack_ragged(items)
        channels = torch.tensor([1 if it[0].ndim == 2 else 3 for it in items], dtype=torch.int32)
        src, d_rgb = buf.to(dev), desc.clone()
        d_rgb[:, 3] = channels
        d_rgb = d_rgb.pin_memory()
        res[name] = dict(timed(lambda: ops.resize_batch_rgb(src, d_rgb, S, out, ws)), source_mb=round(buf.numel() / 1e6, 2))
        first = out.clone()
        if not gray_every:
            d_c3 = desc.pin_memory()
            res["resize_batch_c3_same_batch"] = timed(lambda: ops.resize_batch(src, d_c3, S, 3, out, None, ws))
            res["same_bits_as_resize_batch"] = bool(torch.equal(first.view(torch.int32), out.view(torch.int32)))
    return res


def write_tree(root, n):
    """n JPEG files under root/ft/medpix_dataset (every fourth gray), their csv, and root/data.pt: what Pillow makes of the same files on the host."""
    from PIL import Image
    from src.datasets import captions as C
    folder = os.path.join(root, "ft", "medpix_dataset")
    os.makedirs(os.path.join(folder, "images"))
    base = [speckle(H, W, 3, i)[0] for i in range(16)]
    rng = np.random.default_rng(0)
    rows = []
    for i in range(n):
        px = np.roll(base[i % 16], (i * 7) % H, axis=0)
        name = f"p{i:05d}.jpg"
        Image.fromarray(px[..., 0] if i % 4 == 3 else px, "L" if i % 4 == 3 else "RGB").save(os.path.join(folder, "images", name), quality=90)
        rows.append((" ".join(WORDS[int(j)] for j in rng.integers(0, len(WORDS), 12)), name))
    with open(os.path.join(folder, "medpix_dataset.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Caption", "filename"])
        w.writerows(rows)
    pairs = C.read_pairs(os.path.join(root, "ft"))
    t_decode, t_full, images = [], [], []
    geom = C.geometry(W, H, S)
    for k, (_, path) in enumerate(pairs):
        t0 = time.perf_counter()
        im = Image.open(path)
        im.load()
        t1 = time.perf_counter()
        im = im.convert("RGB").resize((geom[1], geom[0]), Image.BICUBIC).crop((geom[3], geom[2], geom[3] + S, geom[2] + S))
        t2 = time.perf_counter()
        images.append(np.asarray(im).transpose(2, 0, 1))
        if k < 256:
            t_decode.append((t1 - t0) * 1e3)
            t_full.append((t2 - t0) * 1e3)
    # --data_pt takes its validation part from the front; the same 90 / 10 sizes as the folder path
    torch.save({"images": torch.from_numpy(np.stack(images)), "texts": [c for c, _ in pairs]}, os.path.join(root, "data.pt"))
    return {"decode_ms_per_file_one_core": round(statistics.median(t_decode), 3), "decode_resize_crop_ms_per_file_one_core": round(statistics.median(t_full), 3)}


def child(args):
    from src.models.biomedclip import finetune
    source = ["--finetune_root", os.path.join(args.child, "ft")] if args.source == "root" else ["--data_pt", os.path.join(args.child, "data.pt")]
    os.chdir(args.child)
    out = finetune.main(source + ["--method", "mona", "--epochs", "2", "--batch_size", str(args.batch_size), "--num_workers", str(args.num_workers), "--patience", "100",
                                  "--exp", "timing_" + args.source])
    e = out["epochs"][1]
    e["pictures_per_s"] = round(e["batches"] * args.batch_size / (e["ms"] / 1e3), 1)
    print("EPOCH " + json.dumps(e))


def time_loop(args):
    res = {}
    with tempfile.TemporaryDirectory() as root:
        res["host"] = write_tree(root, args.files)
        for source in ("root", "pt"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--source", source, "--num_workers", str(args.num_workers),
                                "--batch_size", str(args.batch_size)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(r.stdout[-2000:] + r.stderr[-4000:])
            res[f"data_{source}_w{args.num_workers}"] = json.loads([line for line in r.stdout.splitlines() if line.startswith("EPOCH ")][-1][6:])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--child", type=str, default=None)
    ap.add_argument("--source", type=str, default="root")
    ap.add_argument("--num_workers", type=int, default=8)
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = {"loop": time_loop(args)} if args.loop else {"launch_b256_500x375_to_298x224_window": time_launches(args)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
