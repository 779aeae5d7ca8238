"""The cost of uia_seg_predict_native (reported in DESIGN.md §4 "Prediction") beside the per-image host loop it replaces.

  launch: ops.seg_predict_native on a batch of --batch 480 x 640 pictures under S = 224 logits, masks and overlays: HIP events around one call (the
          descriptor copy, the statistics' initial value and the kernel), the median of --reps calls after --warmup.
  bytes:  what the call has to move, counted from the shapes (both logit planes once, every source byte once, every mask and overlay byte once), and
          that over the launch time as a share of the HBM peak.
  host:   the same logits through the loop a user would write: per image F.interpolate + argmax on the device, one .cpu() each, the overlay with
          numpy; a host clock around the whole batch (it ends in the last .cpu()), the median of three passes.
  e2e:    (--e2e) the wall time of `python -m src.models.predict` as a child process on --files 480 x 640 pictures with the UNet baseline at img_size
          224 and a checkpoint of its random initialisation, against its number of images.

Prints one JSON line, with the device's clock and power as rocm-smi reports them right after the timed launches."""
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
import torch.nn.functional as F  # noqa: E402

HBM_PEAK = 8.0e12                                                # bytes / s, the MI355X's specified peak


def device_state():
    """Clock and power as rocm-smi reports them (read only); what could not be read is said so."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=60)
        card = next(iter(json.loads(r.stdout).values()))
        return {k: v for k, v in card.items() if "sclk" in k.lower() or "mclk" in k.lower() or "power" in k.lower()}
    except Exception as e:                                       # the figure is context, not a result
        return {"not_read": repr(e)}


def time_launch(args):
    from uia_hip import ops
    from src.utils.viz import NativeMaskWriter
    dev = torch.device("cuda:0")
    B, S, H, W = args.batch, 224, 480, 640
    g = torch.Generator().manual_seed(0)
    logits = (3 * torch.randn(B, 2, S, S, generator=g)).to(dev)
    src = torch.randint(0, 256, (B * H * W,), dtype=torch.uint8, generator=g).to(dev)
    where, total = NativeMaskWriter.layout([(H, W)] * B, overlay=True)
    desc = torch.tensor([[b * H * W, H, W, moff, ooff, 0, 0, 0] for b, (moff, ooff) in enumerate(where)], dtype=torch.int32).pin_memory()
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    stats = torch.empty(B, 8, dtype=torch.int32, device=dev)
    fn = lambda: ops.seg_predict_native(logits, src, desc, out, stats)
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
    state = device_state()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    moved = logits.numel() * 4 + src.numel() + total
    flat, src_host = out.cpu().numpy(), src.cpu().numpy()

    def host_loop():
        masks = []
        for b in range(B):
            up = F.interpolate(logits[b:b + 1], size=(H, W), mode="bilinear", align_corners=False)
            mask = (up.argmax(dim=1)[0].to(torch.uint8) * 255).cpu().numpy()
            gray = src_host[b * H * W:(b + 1) * H * W].reshape(H, W)
            masks.append((mask, np.stack([gray, np.maximum(gray, mask), gray], axis=-1)))
        return masks
    host_loop()
    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        masks = host_loop()
        host.append((time.perf_counter() - t0) * 1e3)
    differ = sum(int((flat[moff:moff + H * W].reshape(H, W) != m).sum()) for (moff, _), (m, _) in zip(where, masks))
    same_overlay = True                                          # the kernel's overlay against numpy's, from the kernel's own mask
    for b, (moff, ooff) in enumerate(where):
        mask, gray = flat[moff:moff + H * W].reshape(H, W), src_host[b * H * W:(b + 1) * H * W].reshape(H, W)
        same_overlay &= np.array_equal(flat[ooff:ooff + 3 * H * W].reshape(H, W, 3), np.stack([gray, np.maximum(gray, mask), gray], axis=-1))
    med = statistics.median(ms)
    return {"batch": B, "S": S, "H": H, "W": W, "reps": args.reps, "launch_ms": round(med, 4), "min": round(ms[0], 4), "max": round(ms[-1], 4),
            "moved_mb": round(moved / 1e6, 2), "share_of_hbm_peak": round(moved / (med * 1e-3) / HBM_PEAK, 4), "host_loop_ms": round(statistics.median(host), 2),
            "mask_pixels_differing_from_torch_fp32": differ, "of": B * H * W, "overlays_equal": bool(same_overlay), "device": state}


def time_e2e(args):
    from PIL import Image
    from src.models.baselines import segmentation as entry
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "pics"))
        rng = np.random.default_rng(0)
        for i in range(args.files):
            Image.fromarray(rng.integers(0, 256, size=(480, 640), dtype=np.uint8)).save(os.path.join(root, "pics", f"p{i:04d}.png"))
        a = entry.get_args(["--device", "cpu"])
        torch.save(entry.prepare_model(a).checkpoint_dict(), os.path.join(root, "w.pth"))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "nextgen-uia_amd"), ROOT]))
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, "-m", "src.models.predict", "--entry", "baselines.segmentation", "--images", "pics", "--out", "out", "--checkpoint", "w.pth",
                            "--", "--batch_size", "32", "--num_workers", "8"], cwd=root, env=env, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-4000:])
        inner = json.loads(r.stdout.strip().splitlines()[-1])
    return {"images": args.files, "process_wall_s": round(wall, 2), "inside_run_s": inner["seconds"], "ms_per_image_wall": round(wall * 1e3 / args.files, 2)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--e2e", action="store_true")
    p.add_argument("--files", type=int, default=256)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_seg_native.py measures on the MI355X: no GPU here, nothing measured")
    res = {"launch": time_launch(args)}
    if args.e2e:
        res["e2e"] = time_e2e(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
