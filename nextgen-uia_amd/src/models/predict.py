"""Prediction on pictures without labels: a trained supervised entry applied to a directory of images, at each image's own size.

    python -m src.models.predict --entry biomedclip.segmentation --images DIR --out DIR [--checkpoint FILE] [--no-overlay] -- <that entry's own flags>
    python -m src.models.predict ... --ensemble SEED2.pth SEED3.pth --tta flips --threshold 0.4 --prob --spread -- <that entry's own flags>

--entry names a module src.models.<family>.<segmentation|classification> (ENTRIES below: the supervised entries, CLIPSeg with its per-batch prompt);
everything else — the few-shot, fine-tune, zero-shot and retrieval modules, a module that does not exist — is refused by name before a model is built.
Everything after `--` goes to the entry's own get_args; the model is its prepare_model(args); the checkpoint defaults to
runs/<exp>/<dataset>/train/best_model.pth, the file the entry's test() loads, and is loaded the same way (model.load_checkpoint, UF.WEIGHTS.bump(),
eval(), no_grad).  A missing image directory or checkpoint and an OUT that is not empty are refused before the GPU is initialised.

Segmentation, per batch: folder.RaggedPrefetcher -> folder.ResizeStage (PIL's resize on the device) -> the task's to_input -> the model -> ONE launch of
uia_hip.ops.seg_predict_native on the batch's own ragged bytes (the S x S logits upsampled to every image's H x W, arg-max, mask, overlay, statistics) ->
one pinned copy back -> at most four writer threads (src/utils/viz.NativeMaskWriter):
    OUT/masks/<stem>.png       8-bit grey, the image's own size        OUT/overlays/<stem>.png    RGB, unless --no-overlay
    OUT/predictions.csv        name,width,height,foreground_pixels,foreground_fraction,ymin,xmin,ymax,xmax   (the box columns empty for an empty mask)
Classification: softmax of the [B, 2] logits on the device, one host copy at the end, OUT/predictions.csv: name,width,height,p0,p1,predicted.
Rows come in file-name order.  No metric is computed and no label is read.  One process, one GPU.

Segmentation only: --min_area N (components below N pixels leave the mask), --keep_largest K (only the K largest stay), --connectivity {4,8} and
--lesions K (0 .. 32) label the masks on the device (uia_hip.ops.mask_components, one call per batch behind the launch above) before they are copied
back: masks, overlays and predictions.csv then describe the filtered mask, and with --lesions K > 0
    OUT/lesions.csv            name,lesion,area,ymin,xmin,ymax,xmax,cy,cx     one row per kept component, at most K per picture, largest first, numbered
                                                                              from 1 (equal areas: the one whose first pixel comes first); none for an empty mask

--close_radius R, --open_radius R (0 .. 64) and --fill_holes N (0 off, -1 any size, N > 0 holes of at most N pixels) reshape the masks on the device
first (uia_hip.ops.mask_morphology, one call per batch between the mask launch and the component call): a closing with the disk of radius R, the holes
of the result filled, then an opening; a hole's connectivity is the complement of --connectivity (12 - it).  Masks, overlays, predictions.csv and
lesions.csv then describe the reshaped mask, and predictions.csv gains the trailing columns pixels_added,pixels_removed.  Segmentation only.

Ensembles: --ensemble FILE [FILE ...] names further checkpoints beside --checkpoint, each loaded into its own prepare_model instance by load_model (a
missing file is refused before the GPU is initialised); --tta {none,hflip,vflip,flips} runs every checkpoint on the S x S model input as it is and
flipped (torch.flip behind the task's to_input): identity; identity and horizontal; identity and vertical; identity, horizontal, vertical and both.
Members = checkpoints x flips, checkpoint-major; more than 16 are refused by name before anything of the entry is imported.  Classification averages
the members' softmax; its CSV header does not change.  Segmentation makes ONE launch of uia_hip.ops.seg_predict_native_ens per batch in place of the
launch above: every member's logits are un-flipped and upsampled to the image's own size, p_k = sigmoid(u_1 - u_0), P = their mean, the mask is
255 where P > --threshold T (default 0.5, 0 < T < 1), and
    OUT/probs/<stem>.png       with --prob: 8-bit grey, round(255 P)          OUT/spread/<stem>.png      with --spread: 8-bit grey, round(255 (max_k p_k - min_k p_k))
--threshold, --prob and --spread are for segmentation only.  When any of the five flags is given, predictions.csv of a segmentation entry gains two
trailing columns, six decimals each: mean_foreground_probability = the sum of the probability bytes over the UNFILTERED mask / (255 x its pixels), empty
for an empty mask, and mean_spread = the sum of the spread bytes / (255 x H x W).  Without them the old launch runs and the old bytes are written.
"""
import argparse
import importlib
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import torch

ENTRIES = {"baselines": ("classification", "segmentation"), "biomedclip": ("classification", "segmentation"), "clip": ("classification", "segmentation"),
           "clipseg": ("segmentation",), "dino": ("classification", "segmentation"), "metaclip": ("classification", "segmentation"),
           "unimedclip": ("classification", "segmentation")}
SEG_HEADER = "name,width,height,foreground_pixels,foreground_fraction,ymin,xmin,ymax,xmax"
CLS_HEADER = "name,width,height,p0,p1,predicted"
LESION_HEADER = "name,lesion,area,ymin,xmin,ymax,xmax,cy,cx"
MAX_LESIONS = 32
ENS_COLUMNS = "mean_foreground_probability,mean_spread"
MAX_MEMBERS = 16
TTA_FLIPS = {"none": (0,), "hflip": (0, 1), "vflip": (0, 2), "flips": (0, 1, 2, 3)}      # bit 0: the input is flipped horizontally, bit 1: vertically
ENSEMBLE_FLAGS = {"ensemble": ("--ensemble", None), "tta": ("--tta", "none"), "threshold": ("--threshold", 0.5), "prob": ("--prob", False),
                  "spread": ("--spread", False)}
SEG_ONLY_FLAGS = ("threshold", "prob", "spread")
MORPH_COLUMNS = "pixels_added,pixels_removed"
MAX_RADIUS = 64
MORPHOLOGY_FLAGS = {"close_radius": ("--close_radius", 0), "open_radius": ("--open_radius", 0), "fill_holes": ("--fill_holes", 0)}
COMPONENT_FLAGS = {"min_area": ("--min_area", 0), "keep_largest": ("--keep_largest", 0), "connectivity": ("--connectivity", 8), "lesions": ("--lesions", 0)}


def split_argv(argv):
    """argv -> (this module's arguments, the entry's own): the split at the first `--`."""
    argv = list(argv)
    if "--" in argv:
        at = argv.index("--")
        return argv[:at], argv[at + 1:]
    return argv, []


def get_args(argv=None):
    own, rest = split_argv(sys.argv[1:] if argv is None else argv)
    p = argparse.ArgumentParser("Masks or class probabilities for a directory of images, from a trained supervised entry")
    p.add_argument("--entry", type=str, required=True, help="<family>.<segmentation|classification>, e.g. biomedclip.segmentation")
    p.add_argument("--images", type=str, required=True, help="directory of .png .jpg .jpeg .bmp .tif .tiff files (not read recursively)")
    p.add_argument("--out", type=str, required=True, help="output directory; must be absent or empty")
    p.add_argument("--checkpoint", type=str, default=None, help="default: runs/<exp>/<dataset>/train/best_model.pth of the entry's flags")
    p.add_argument("--overlay", default=True, action=argparse.BooleanOptionalAction, help="segmentation: write OUT/overlays/<stem>.png")
    p.add_argument("--min_area", type=int, default=0, help="segmentation: components of fewer pixels leave the mask (0 or 1: none does)")
    p.add_argument("--keep_largest", type=int, default=0, help="segmentation: only the K largest components stay (0: any number)")
    p.add_argument("--connectivity", type=int, default=8, choices=(4, 8), help="segmentation: what joins two pixels into one component")
    p.add_argument("--lesions", type=int, default=0, help=f"segmentation: write OUT/lesions.csv with the K <= {MAX_LESIONS} largest kept components of every picture")
    p.add_argument("--close_radius", type=int, default=0, help=f"segmentation: close the mask with a disk of radius R (0 .. {MAX_RADIUS}; 0: off)")
    p.add_argument("--open_radius", type=int, default=0, help=f"segmentation: open the mask with a disk of radius R (0 .. {MAX_RADIUS}; 0: off), after closing and filling")
    p.add_argument("--fill_holes", type=int, default=0, help="segmentation: fill the holes of the closed mask (0: off, -1: any size, N > 0: holes of at most N pixels)")
    p.add_argument("--ensemble", type=str, nargs="+", default=None, metavar="FILE", help="further checkpoints beside --checkpoint, averaged with it")
    p.add_argument("--tta", type=str, default="none", choices=tuple(TTA_FLIPS), help="flips of the model input every checkpoint is run on: identity; identity "
                   f"and horizontal; identity and vertical; all four.  Members = checkpoints x flips, at most {MAX_MEMBERS}")
    p.add_argument("--threshold", type=float, default=0.5, help="segmentation: the mask is 255 where the mean foreground probability exceeds T, 0 < T < 1")
    p.add_argument("--prob", default=False, action="store_true", help="segmentation: write OUT/probs/<stem>.png, the mean foreground probability as 8-bit grey")
    p.add_argument("--spread", default=False, action="store_true", help="segmentation: write OUT/spread/<stem>.png, max - min of the members' probabilities")
    return p.parse_args(own), rest


def ensemble_given(own):
    """The new flags that differ from their defaults, by name: with none of them prediction runs exactly as it did before they existed."""
    return [flag for key, (flag, default) in ENSEMBLE_FLAGS.items() if getattr(own, key) != default]


def members_of(own):
    """-> [(checkpoint index, flip)]: checkpoints (--checkpoint, then --ensemble in the order given) x flips of --tta, checkpoint-major."""
    return [(c, f) for c in range(1 + len(own.ensemble or ())) for f in TTA_FLIPS[own.tta]]


def check_ensemble(own, kind):
    """The ensemble flags within the kernel's limits and the segmentation-only ones on a segmentation entry: refused by name before anything of the entry
    is imported."""
    given = [ENSEMBLE_FLAGS[key][0] for key in SEG_ONLY_FLAGS if getattr(own, key) != ENSEMBLE_FLAGS[key][1]]
    if kind != "segmentation" and given:
        raise ValueError(f"--entry {own.entry}: {', '.join(given)} shape segmentation masks and maps; a classification entry has none")
    if not 0.0 < own.threshold < 1.0:
        raise ValueError(f"--threshold {own.threshold}: 0 < T < 1")
    n = len(members_of(own))
    if n > MAX_MEMBERS:
        raise ValueError(f"--ensemble / --tta: {1 + len(own.ensemble or ())} checkpoints x {len(TTA_FLIPS[own.tta])} flips = {n} members, at most {MAX_MEMBERS}")


def check_components(own, kind):
    """The component flags are for segmentation and within the kernel's limits: refused by name before anything of the entry is imported."""
    given = [flag for key, (flag, default) in COMPONENT_FLAGS.items() if getattr(own, key) != default]
    if kind != "segmentation" and given:
        raise ValueError(f"--entry {own.entry}: {', '.join(given)} filter segmentation masks; a classification entry has none")
    if own.min_area < 0 or own.keep_largest < 0:
        raise ValueError(f"--min_area {own.min_area} / --keep_largest {own.keep_largest}: neither may be negative")
    if not 0 <= own.lesions <= MAX_LESIONS:
        raise ValueError(f"--lesions {own.lesions}: 0 .. {MAX_LESIONS}")


def morphology_given(own):
    """The morphology flags that differ from their defaults, by name: with none of them nothing else is enqueued and predictions.csv keeps its columns."""
    return [flag for key, (flag, default) in MORPHOLOGY_FLAGS.items() if getattr(own, key) != default]


def check_morphology(own, kind):
    """The morphology flags are for segmentation and within the kernel's limits: refused by name before anything of the entry is imported."""
    given = morphology_given(own)
    if kind != "segmentation" and given:
        raise ValueError(f"--entry {own.entry}: {', '.join(given)} reshape segmentation masks; a classification entry has none")
    for key in ("close_radius", "open_radius"):
        if not 0 <= getattr(own, key) <= MAX_RADIUS:
            raise ValueError(f"--{key} {getattr(own, key)}: 0 .. {MAX_RADIUS}")
    if own.fill_holes < -1:
        raise ValueError(f"--fill_holes {own.fill_holes}: 0 (off), -1 (any size) or the largest hole filled, in pixels")


def entry_kind(name):
    """"<family>.<kind>" -> (family, kind), or the refusal, by name."""
    family, _, kind = str(name).partition(".")
    if kind not in ENTRIES.get(family, ()):
        known = ", ".join(f"{f}.{k}" for f, kinds in ENTRIES.items() for k in kinds)
        raise ValueError(f"--entry {name}: prediction runs the supervised classification and segmentation entries only ({known}); the few-shot, fine-tune, "
                         "zero-shot and retrieval modules have no checkpoint of that form")
    return family, kind


def default_checkpoint(entry_args):
    return f"runs/{entry_args.exp}/{entry_args.dataset}/train/best_model.pth"


def seg_csv(names, sizes, stats, sums=None, filtered=False, morphology=None):
    """names, [(H, W)], stats rows (foreground pixels, ymin, xmin, ymax, xmax, ...) -> the text of predictions.csv.  With sums rows (sum of the
    probability bytes over the launch's own mask, sum of the spread bytes) the two ensemble columns follow; `filtered` says that the stats are
    uia_mask_components', whose word 7 is the foreground before the filter.  With morphology rows (pixels added, pixels removed, foreground of the
    launch's own mask: uia_mask_morphology's words 5-7) the two morphology columns come last, and the ensemble column's denominator is those rows'
    third word: behind a morphology call the component filter's word 7 counts the morphology's result, not the launch's mask."""
    lines = [",".join([SEG_HEADER] + ([ENS_COLUMNS] if sums is not None else []) + ([MORPH_COLUMNS] if morphology is not None else []))]
    for i, (name, (H, W), s) in enumerate(zip(names, sizes, stats)):
        n, box = int(s[0]), ",".join(str(int(v)) for v in s[1:5]) if int(s[0]) > 0 else ",,,"
        line = f"{name},{W},{H},{n},{n / (H * W):.6f},{box}"
        if sums is not None:
            before = int(morphology[i][2]) if morphology is not None else (int(s[7]) if filtered else n)
            line += f",{int(sums[i][0]) / (255 * before):.6f}" if before > 0 else ","
            line += f",{int(sums[i][1]) / (255 * H * W):.6f}"
        if morphology is not None:
            line += f",{int(morphology[i][0])},{int(morphology[i][1])}"
        lines.append(line)
    return "\n".join(lines) + "\n"


def lesions_csv(names, lists):
    """names, per image rows (area, ymin, xmin, ymax, xmax, first pixel, cy, cx) with zero rows unused -> the text of lesions.csv: one row per kept
    component, numbered from 1 in the kernel's order; a picture without one gets no row."""
    lines = [LESION_HEADER]
    for name, rows in zip(names, lists):
        for k, r in enumerate(rows):
            if int(r[0]) <= 0:
                break
            lines.append(f"{name},{k + 1},{int(r[0])},{int(r[1])},{int(r[2])},{int(r[3])},{int(r[4])},{int(r[6])},{int(r[7])}")
    return "\n".join(lines) + "\n"


def cls_csv(names, sizes, probs):
    """names, [(H, W)], probabilities [n][2] -> the text of predictions.csv; `predicted` is the arg-max (a tie goes to class 0, as torch.argmax)."""
    lines = [CLS_HEADER]
    for name, (H, W), (p0, p1) in zip(names, sizes, probs):
        lines.append(f"{name},{W},{H},{float(p0):.8f},{float(p1):.8f},{1 if float(p1) > float(p0) else 0}")
    return "\n".join(lines) + "\n"


def load_model(module, entry_args, checkpoint):
    """The entry's model with the checkpoint in it, as its test() prepares it."""
    from uia_hip import functional as UF
    model = module.prepare_model(entry_args)
    model.load_checkpoint(torch.load(checkpoint, map_location="cpu"))
    UF.WEIGHTS.bump()
    model.eval()
    return model


@torch.no_grad()
def run(own, entry_args, module, kind):
    from src.datasets import folder
    from src.datasets.image_dir import ImageDirModule
    from src.models import supervised
    from src.utils.viz import NativeMaskWriter
    from uia_hip import functional as UF

    t0 = time.perf_counter()
    seg = kind == "segmentation"
    task = getattr(module, "TASK", supervised.SEGMENTATION if seg else supervised.CLASSIFICATION)
    checkpoint = own.checkpoint or default_checkpoint(entry_args)
    if not os.path.isdir(own.images):
        raise FileNotFoundError(f"--images {own.images}: no such directory")
    if os.path.exists(own.out) and (not os.path.isdir(own.out) or os.listdir(own.out)):
        raise FileExistsError(f"--out {own.out} exists and is not an empty directory: nothing is overwritten")
    if not os.path.isfile(checkpoint):
        raise FileNotFoundError(f"checkpoint {checkpoint} not found (train the entry first, or pass --checkpoint)")
    for extra in own.ensemble or ():
        if not os.path.isfile(extra):
            raise FileNotFoundError(f"--ensemble {extra} not found")
    extended, members = bool(ensemble_given(own)), members_of(own)
    if hasattr(module, "check_args"):
        module.check_args(entry_args)
    dm = ImageDirModule(own.images, entry_args.img_size, entry_args.batch_size, getattr(entry_args, "num_workers", 0))
    dm.start_workers()                                           # loader worker processes are forked BEFORE this process touches the GPU
    ds = dm.dataset

    torch.cuda.set_device(torch.device(entry_args.device))
    UF.set_compute_dtype(torch.bfloat16 if entry_args.dtype == "bf16" else torch.float32)
    models = [load_model(module, entry_args, c) for c in [checkpoint] + list(own.ensemble or ())]
    model = models[0]
    prompt = getattr(module, "_batch_prompt", None)              # CLIPSeg: the per-batch prompt keyword function its test() hands to the loop
    kwargs_for = prompt(entry_args) if prompt is not None else (lambda n: {})
    os.makedirs(own.out, exist_ok=True)
    writer = NativeMaskWriter(own.out, overlay=own.overlay, min_area=own.min_area, keep=own.keep_largest, connectivity=own.connectivity,
                              lesions=own.lesions, threshold=own.threshold, prob=own.prob, spread=own.spread, close_radius=own.close_radius,
                              open_radius=own.open_radius, fill_holes=own.fill_holes) if seg else None
    pf = folder.RaggedPrefetcher(dm.loader, entry_args.device)
    resize = folder.ResizeStage(entry_args.img_size, with_mask=seg)
    cur = torch.cuda.current_stream()
    seen, probs, batches, lists, sums, morph = 0, [], [], [], [], []
    try:
        for batch, second, ready in pf:
            cur.wait_event(ready)
            n = batch.desc.shape[0]
            names = [ds.name_of(seen + j) for j in range(n)]    # the prefetcher drops names; the loader does not shuffle
            seen += n
            images, second = resize(batch, second)
            images, _ = task.to_input(images, second, entry_args.in_channels)
            if not extended:
                logits = model(images, **kwargs_for(n)).detach()
                if seg:
                    writer.submit(logits, batch, names)
                else:
                    probs.append(torch.softmax(logits.float(), dim=1))
                continue
            flipped = {f: images if f == 0 else torch.flip(images, dims=[d for d, bit in ((-1, 1), (-2, 2)) if f & bit]) for f in TTA_FLIPS[own.tta]}
            stack = torch.stack([models[c](flipped[f], **kwargs_for(n)).detach().float() for c, f in members])
            if seg:
                writer.submit(stack, batch, names, flips=[f for _, f in members])
            else:
                probs.append(torch.softmax(stack, dim=2).mean(dim=0))
        if seg:
            batches, lists, sums, morph, writer = writer.close(), writer.lesion_lists(), writer.sums(), writer.morphology_stats(), None     # the writers are joined; a writer's exception surfaces here
    finally:
        if writer is not None:
            writer.close()
        pf.close()
        dm.shutdown()
    sizes = [(H, W) for W, H in ds.sizes]
    if seg:
        done = [name for b in batches for name in b[0]]
        assert done == ds.names, "a batch is missing from the writers' results"
        text = seg_csv(ds.names, sizes, [row for b in batches for row in b[2]], [row for b in sums for row in b] if extended else None,
                       filtered=(own.min_area, own.keep_largest, own.connectivity, own.lesions) != (0, 0, 8, 0),
                       morphology=[row for b in morph for row in b] if morphology_given(own) else None)
        if own.lesions > 0:
            with open(os.path.join(own.out, "lesions.csv"), "w") as f:
                f.write(lesions_csv(ds.names, [rows for b in lists for rows in b]))
    else:
        text = cls_csv(ds.names, sizes, torch.cat(probs).cpu().tolist())
    with open(os.path.join(own.out, "predictions.csv"), "w") as f:
        f.write(text)
    return {"entry": own.entry, "images": len(ds), "out": own.out, "checkpoint": checkpoint, "seconds": round(time.perf_counter() - t0, 3)}


def main(argv=None):
    own, rest = get_args(argv)
    family, kind = entry_kind(own.entry)                         # refused by name before anything of the entry is imported or built
    check_components(own, kind)
    check_morphology(own, kind)
    check_ensemble(own, kind)
    module = importlib.import_module(f"src.models.{family}.{kind}")
    entry_args = module.get_args(rest)
    out = run(own, entry_args, module, kind)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
