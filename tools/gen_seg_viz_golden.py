"""Writes tests/golden/seg_viz_cases.npz: small inputs and what the reference's own visualize_seg (src/utils/tools.py) made of them, decoded from the PNG
files it wrote.  Data only: the reference module is imported from its tree and called; none of its text is stored.

    python tools/gen_seg_viz_golden.py REFERENCE_DIR

The reference module imports torchmetrics and monai.metrics at its top, which visualize_seg never touches; where they are absent, stand-in modules are
installed before the import.  Cases (B = 3 each): S = 5 and S = 37, three-channel and one-channel images holding every level k / 255 (both as
arange(256, float32) / 255 and as uint8.float() / 255.0) plus 1.0 and 0.999999, float and uint8 labels with one all-empty and one all-full mask, logits
with planted exact ties, -0.0 against +0.0 and +-inf.  No out-of-range pixel and no NaN logit: the reference's behaviour there is not a contract.
"""
import importlib
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Anything:
    """Callable, attribute-bearing nothing: what the module-level metric objects of the reference module become."""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return self

    def __getattr__(self, name):
        return self


def _stand_in(name, attrs):
    try:
        importlib.import_module(name)
        return
    except ImportError:
        pass
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
    for a in attrs:
        setattr(sys.modules[name], a, _Anything)


def load_reference_tools(reference_dir):
    _stand_in("torchmetrics", ["Accuracy", "Precision", "Recall", "F1Score", "AUROC", "ROC"])
    _stand_in("monai.metrics", ["compute_dice", "compute_iou", "compute_hausdorff_distance", "compute_average_surface_distance", "PSNRMetric", "SSIMMetric"])
    import matplotlib
    matplotlib.use("Agg")
    spec = importlib.util.spec_from_file_location("reference_tools", os.path.join(reference_dir, "src/utils/tools.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def levels(n, g):
    """n pixel values in [0, 1]: the 256 levels both ways, 1.0 and 0.999999 first, the rest uniform; cut to n when n is small."""
    a = np.arange(256, dtype=np.float32) / np.float32(255)
    b = (torch.arange(256, dtype=torch.uint8).float() / 255.0).numpy()
    head = np.concatenate([np.float32([1.0, 0.999999, 0.0]), a[::-1], b])
    if n <= head.size:
        return np.concatenate([head[:3], a[np.linspace(0, 255, n - 3).astype(int)]]).astype(np.float32)
    return np.concatenate([head, torch.rand(n - head.size, generator=g).numpy()]).astype(np.float32)


def make_case(S, Ci, label_dtype, seed):
    g = torch.Generator().manual_seed(seed)
    B, n = 3, S * S
    images = np.empty((B, Ci, S, S), dtype=np.float32)
    for b in range(B):
        for c in range(Ci):
            v = levels(n, g)
            images[b, c] = v[torch.randperm(n, generator=g).numpy()].reshape(S, S)       # channel 0 is drawn: the others differ on purpose
    labels = np.zeros((B, 1, S, S), dtype=np.float32)
    labels[0, 0] = (torch.rand(S, S, generator=g) < 0.4).numpy()
    labels[2] = 1.0                                              # image 1: all empty, image 2: all full
    logits = torch.randn(B, 2, S, S, generator=g).numpy()
    flat = logits.reshape(B, 2, n)
    k = torch.randperm(n, generator=g).numpy()
    inf = np.float32(np.inf)
    plant = [(1.5, 1.5), (0.0, -0.0), (-0.0, 0.0), (inf, inf), (-inf, -inf), (inf, 1.0), (1.0, inf), (-inf, 1.0), (1.0, -inf), (-inf, inf), (inf, -inf)]
    for b in range(B):
        for j, (l0, l1) in enumerate(plant):
            flat[b, 0, k[(j + 3 * b) % n]], flat[b, 1, k[(j + 3 * b) % n]] = l0, l1
    return logits.astype(np.float32), images, labels.astype(label_dtype)


def main(reference_dir):
    from PIL import Image
    ref = load_reference_tools(reference_dir)
    out, names = {}, [f"dir/sample_{i}.png" for i in range(3)]
    cases = [(37, 3, np.float32), (37, 1, np.uint8), (5, 3, np.uint8), (5, 1, np.float32)]
    for c, (S, Ci, dt) in enumerate(cases):
        logits, images, labels = make_case(S, Ci, dt, 100 + c)
        with tempfile.TemporaryDirectory() as td:
            ref.visualize_seg(torch.from_numpy(images), torch.from_numpy(labels), torch.from_numpy(logits), names, td)
            assert sorted(os.listdir(td)) == sorted(f"sample_{i}{s}.png" for i in range(3) for s in ("", "_overlay", "_pred")), os.listdir(td)
            read = lambda suffix: np.stack([np.asarray(Image.open(f"{td}/sample_{i}{suffix}.png")) for i in range(3)])
            mask, overlay, pred = read(""), read("_overlay"), read("_pred")
        assert mask.shape == (3, S, S, 3) and overlay.shape == (3, S, S, 3) and pred.shape == (3, S, S) and pred.dtype == np.uint8
        out.update({f"c{c}_logits": logits, f"c{c}_images": images, f"c{c}_labels": labels, f"c{c}_mask": mask, f"c{c}_overlay": overlay, f"c{c}_pred": pred})
    path = os.path.join(ROOT, "tests/golden/seg_viz_cases.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
