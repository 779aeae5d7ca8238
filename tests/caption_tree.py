"""A small tree in the layout of the reference's caption folders, written with Pillow, for tests/test_captions_host.py and tests/test_captions_gpu.py:
24 valid image-caption pairs over the two datasets — "L", "RGB", "P" and "RGBA" PNG files and JPEG files, landscape, portrait and square, one file
above the loader's per-image byte limit — plus the rows the preparation must drop or mend, and the seven-word tokenizer file the tests encode with."""
import csv
import os

import numpy as np

WORDS = ["lesion", "scan", "of", "the", "liver", "shows", "mass"]
VOCAB = {"[PAD]": 0, "[UNK]": 1, "[CLS]": 2, **{w: 3 + i for i, w in enumerate(WORDS)}, "[SEP]": 10}      # the end token is the largest id
MODES = ["L", "RGB", "P", "RGBA", "JPEG"]
BIG = "big_00.png"                                              # 1100 x 1000 gray: 1.1 MB decoded, above captions.IMAGE_LIMIT
N_VALID = 24


def caption_of(i):
    return " ".join(WORDS[(i + k) % 7] for k in range(5 + i % 4))           # 5 .. 8 words, always longer than 20 characters


def size_of(i):
    """(W, H): landscape, portrait and square in turn, 33 .. 75 a side."""
    a, b = 33 + (i * 5) % 29, 47 + (i * 7) % 29
    return [(max(a, b) + 1, min(a, b)), (min(a, b), max(a, b) + 1), (a, a)][i % 3]


def _picture(i, W, H):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rng = np.random.default_rng(100 + i)
    base = (127 + 120 * np.sin(xx / (2.0 + i % 5)) * np.cos(yy / (3.0 + i % 3)))[..., None] + rng.integers(-7, 8, (H, W, 3))
    return np.clip(base + np.array([0, 10, -10]), 0, 255).astype(np.uint8)


def _save(path, i, mode):
    from PIL import Image
    W, H = size_of(i)
    px = _picture(i, W, H)
    if mode == "L":
        Image.fromarray(px[..., 0], "L").save(path)
    elif mode == "RGB":
        Image.fromarray(px, "RGB").save(path)
    elif mode == "P":
        Image.fromarray(px, "RGB").quantize(16).save(path)
    elif mode == "RGBA":
        Image.fromarray(np.concatenate([px, np.full((H, W, 1), 200, np.uint8)], axis=2), "RGBA").save(path)
    else:
        Image.fromarray(px, "RGB").save(path, quality=90)


def write_tree(root, datasets=("medpix_dataset", "pmc_curd_dataset")):
    """-> [(caption as the preparation leaves it, image path)] in csv order (medpix first): what captions.read_pairs must return."""
    from PIL import Image
    root = str(root)
    expect = {d: [] for d in ("medpix_dataset", "pmc_curd_dataset")}
    rows = {d: [] for d in expect}
    for d in datasets:
        os.makedirs(os.path.join(root, d, "images"), exist_ok=True)
    for i in range(N_VALID):
        d = "medpix_dataset" if i < 14 else "pmc_curd_dataset"
        if d not in datasets:
            continue
        mode = MODES[i % 5]
        name = f"pic_{i:02d}.{'jpg' if mode == 'JPEG' else 'png'}"
        if i == 5:
            name = BIG
            yy, xx = np.meshgrid(np.arange(1000), np.arange(1100), indexing="ij")
            Image.fromarray(((xx // 9 + yy // 7) % 256).astype(np.uint8), "L").save(os.path.join(root, d, "images", name))
        else:
            # picture 3's file lies in the OTHER dataset's folder (the lookup goes through both), where there is one
            home = "pmc_curd_dataset" if i == 3 and len(datasets) == 2 else d
            _save(os.path.join(root, home, "images", name), i, mode)
        listed = f"some/prefix/{name}" if i % 6 == 1 else name      # only the basename counts
        raw = caption_of(i)
        if i == 2:
            raw = "  " + raw.replace(" ", " § ", 1) + " ™é  "       # characters the pattern removes, white space the strip removes
            cleaned = caption_of(i).replace(" ", "  ", 1)
        else:
            cleaned = raw
        rows[d].append((raw, listed))
        home = "pmc_curd_dataset" if i == 3 and len(datasets) == 2 else d
        expect[d].append((cleaned, os.path.join(root, home, "images", name)))
    if "medpix_dataset" in datasets:
        rows["medpix_dataset"].insert(4, ("too short", "pic_00.png"))                          # 9 characters
        rows["medpix_dataset"].insert(9, ("exactly twenty chars", "pic_00.png"))               # 20: not LONGER than 20
        rows["medpix_dataset"].append((caption_of(1), "not_there.png"))                        # no such file
    for d in datasets:
        with open(os.path.join(root, d, f"{d}.csv"), "w", newline="", encoding="utf-8") as f:
            w = csv.writer(f)
            w.writerow(["id", "Caption", "filename"])
            w.writerows((k, c, fn) for k, (c, fn) in enumerate(rows[d]))
    return [p for d in ("medpix_dataset", "pmc_curd_dataset") if d in datasets for p in expect[d]]


def write_tokenizer(path, sep_largest=True):
    """The seven-word WordPiece tokenizer with a `[CLS] $A [SEP]` template.  sep_largest False: [CLS] and [SEP] change places, as in a BERT vocabulary."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    vocab = dict(VOCAB)
    if not sep_largest:
        vocab["[SEP]"], vocab["[CLS]"] = vocab["[CLS]"], vocab["[SEP]"]
    tk = Tokenizer(models.WordPiece(vocab=vocab, unk_token="[UNK]"))
    tk.pre_tokenizer = pre_tokenizers.Whitespace()
    tk.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", vocab["[CLS]"]), ("[SEP]", vocab["[SEP]"])])
    tk.save(str(path))
    return str(path)


def pillow_batch(paths, S):
    """What the reference's worker makes of these files: Image.open -> convert("RGB") -> Resize(S, BICUBIC) -> CenterCrop(S) -> / 255, fp32
    [n, 3, S, S], with Pillow alone (the shorter-side rule and the crop written out from torchvision's source)."""
    import torch
    from PIL import Image
    out = []
    for p in paths:
        im = Image.open(p)
        if im.mode != "RGB":
            im = im.convert("RGB")
        W, H = im.size
        if W <= H:
            nw, nh = S, int(S * H / W)
        else:
            nw, nh = int(S * W / H), S
        im = im.resize((nw, nh), Image.BICUBIC)
        top, left = int(round((nh - S) / 2.0)), int(round((nw - S) / 2.0))
        im = im.crop((left, top, left + S, top + S))
        out.append(torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).float() / 255)
    return torch.stack(out)
