"""numpy restatement of the segmentation pictures (uia_seg_viz, include/uia_hip.h): the three rules of the reference's visualize_seg plus the clamp.

    g = (uint8)(x * 255)   one float32 product, clamped to [0, 255] with NaN -> 0, truncated
    t = 255 where label != 0
    p = 255 where class 1 wins the arg-max: l1 > l0, or l1 is NaN and l0 is not (a tie goes to class 0, NaN is the maximum)
    mask_rgb = (t, p, 0), overlay_rgb = (max(g, t), max(g, p), g), pred = p
"""
import numpy as np


def class1(logits):
    """[B, 2, S, S] float32 -> bool [B, S, S]: torch.argmax(dim=1) == 1, restated."""
    l0, l1 = logits[:, 0], logits[:, 1]
    with np.errstate(invalid="ignore"):
        return (l1 > l0) | (np.isnan(l1) & ~np.isnan(l0))


def grey(x):
    v = np.asarray(x, dtype=np.float32) * np.float32(255)
    with np.errstate(invalid="ignore"):
        v = np.where(v > 0, v, np.float32(0))                    # below 0 and NaN -> 0
        v = np.where(v < 255, v, np.float32(255))
    return v.astype(np.uint8)                                    # in range: truncation


def seg_viz(logits, images, labels, pred_class1=None):
    """logits float32 [B, 2, S, S], images float32 [B, Ci, S, S], labels [B, 1, S, S] (any dtype) -> (mask_rgb [B, S, S, 3], overlay_rgb [B, S, S, 3],
    pred [B, S, S]) uint8.  pred_class1: a bool [B, S, S] that takes the place of the restated arg-max (the device's own torch.argmax in the GPU tests)."""
    logits, images, labels = np.asarray(logits), np.asarray(images), np.asarray(labels)
    won = class1(logits) if pred_class1 is None else np.asarray(pred_class1, dtype=bool)
    p = np.where(won, 255, 0).astype(np.uint8)
    t = np.where(labels[:, 0] != 0, 255, 0).astype(np.uint8)
    g = grey(images[:, 0])
    mask = np.stack([t, p, np.zeros_like(t)], axis=-1)
    overlay = np.stack([np.maximum(g, t), np.maximum(g, p), g], axis=-1)
    return mask, overlay, p


def decode_png(data):
    """The bytes of an 8-bit grey or RGB PNG whose rows all carry filter type 0 -> uint8 [H, W] or [H, W, 3] (what src.utils.viz.write_png writes)."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, colour, comp, filt, lace = head
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 2)
    ch = 3 if colour == 2 else 1
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + w * ch)
    assert not rows[:, 0].any(), "a row with a filter type other than 0"
    px = rows[:, 1:]
    return px.reshape(h, w, 3).copy() if ch == 3 else px.copy()
