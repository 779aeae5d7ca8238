"""Writes tests/golden/resize_pil.npz: what Pillow's `Image.resize` gives on the cases of tests/resize_cases.py — "L" / "RGB" images through the default
(antialiased bicubic) filter, mode "1" masks through the default (nearest) one, the S x S window cut out afterwards.  Only the outputs are stored; the
tests regenerate the inputs.  PIL.__version__ is recorded in the file.

    python tools/gen_resize_golden.py
"""
import json
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resize_cases as RC  # noqa: E402


def main():
    out = {"pil_version": np.array(PIL.__version__), "cases": np.array(json.dumps(RC.CASES))}
    for c in RC.CASES:
        px, mask = RC.make_input(c)
        y0, x0, S = c["y0"], c["x0"], c["S"]
        im = Image.fromarray(px, "L" if c["C"] == 1 else "RGB").resize((c["dst_w"], c["dst_h"]))
        out["img_" + c["name"]] = np.asarray(im)[y0:y0 + S, x0:x0 + S].copy()
        if mask is not None:
            mi = Image.fromarray(mask, "L").convert("1").resize((c["dst_w"], c["dst_h"]))
            out["mask_" + c["name"]] = np.asarray(mi, dtype=np.uint8)[y0:y0 + S, x0:x0 + S].copy()
    np.savez_compressed(RC.GOLDEN, **out)
    print(f"{RC.GOLDEN}: {len(RC.CASES)} cases, Pillow {PIL.__version__}, {os.path.getsize(RC.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
