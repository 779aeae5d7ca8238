"""A small dataset tree in the reference's layout, written with Pillow, for tests/test_resize_host.py and tests/test_folder_gpu.py: 12 pictures of
40 to 90 pixels a side (every second one saved as RGB, so that convert("L") is a luma and not a channel pick), their masks, the split lists of a
segmentation and a classification dataset "TOY", and labels.csv.  Also the --data_pt file PIL makes from the same files on the host."""
import os

import numpy as np

NAMES = [f"img_{i:02d}.png" for i in range(12)]
SPLITS = {"train": NAMES[:6], "val": NAMES[6:9], "test": NAMES[9:]}
LABELS = {n: i % 2 for i, n in enumerate(NAMES)}
DATASET = "TOY"


def size_of(i):
    """(W, H) of picture i: 40 .. 90, never square."""
    return 40 + (i * 7) % 51, 90 - (i * 11) % 51


def write_tree(root):
    from PIL import Image
    root = str(root)
    for d in ("all/images", "all/masks", f"segmentation/{DATASET}", f"classification/{DATASET}"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    rng = np.random.default_rng(7)
    for i, n in enumerate(NAMES):
        W, H = size_of(i)
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        blob = ((yy - H / 2) / (H / 3)) ** 2 + ((xx - W / 2) / (W / 4)) ** 2 <= 1
        px = rng.integers(0, 160, (H, W, 3), dtype=np.uint8)
        px[blob] += np.uint8(90) * np.uint8(LABELS[n])           # class 1 carries a bright lesion
        if i % 2:
            Image.fromarray(px, "RGB").save(os.path.join(root, "all/images", n))
        else:
            Image.fromarray(px[..., 0], "L").save(os.path.join(root, "all/images", n))
        Image.fromarray(blob.astype(np.uint8) * 255, "L").save(os.path.join(root, "all/masks", n))
    for kind in ("segmentation", "classification"):
        for split, names in SPLITS.items():
            with open(os.path.join(root, kind, DATASET, f"{split}.txt"), "w") as f:
                f.write("\n".join(names) + "\n")
    with open(os.path.join(root, "classification", DATASET, "labels.csv"), "w") as f:
        f.writelines(f"{n},{v}\n" for n, v in LABELS.items())
    return root


def write_data_pt(root, path, S, kind):
    """What the reference's worker computes on the host before its augmentations — Image.open().convert("L").resize((S, S)), masks .convert("1")
    .resize((S, S)) — as the --data_pt file of this build: uint8 images [N, 1, S, S], masks [N, 1, S, S] or labels [N], names and the split."""
    import torch
    from PIL import Image
    images = np.stack([np.asarray(Image.open(os.path.join(root, "all/images", n)).convert("L").resize((S, S))) for n in NAMES])[:, None]
    if kind == "segmentation":
        labels = np.stack([np.asarray(Image.open(os.path.join(root, "all/masks", n)).convert("1").resize((S, S)), dtype=np.uint8) for n in NAMES])[:, None]
    else:
        labels = np.array([LABELS[n] for n in NAMES], dtype=np.int64)
    split = {k: [NAMES.index(n) for n in v] for k, v in SPLITS.items()}
    torch.save({"images": torch.from_numpy(images.copy()), "labels": torch.from_numpy(labels.copy()), "names": list(NAMES), "split": split}, str(path))
    return str(path)
