"""Host checks of the --finetune_root path (src/datasets/captions.py) and of --tokenizer_json (src/utils/tokenizer_file.py): the Resize + CenterCrop
geometry against live Pillow, the csv preparation on a generated tree (tests/caption_tree.py), the ring of byte slots with forked workers and no
GPU, and the tokenizer file's ids, truncation, padding and refusals."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import caption_tree as T  # noqa: E402

pytest.importorskip("PIL")

# (W, H, S): landscape, portrait, square, a short side equal to S, odd differences whose half rounds to even (4.5 -> 4, 5.5 -> 6), an upscale
GEOMETRY = [(500, 375, 224), (375, 500, 224), (300, 300, 224), (37, 23, 16), (23, 37, 16), (40, 16, 16), (16, 16, 16), (43, 16, 16), (9, 8, 16),
            (640, 427, 224), (33, 100, 32)]


def _args(root=None, **kw):
    base = dict(finetune_root=root, data_pt=None, synthetic=False, data_root=None, img_size=32, batch_size=4, num_workers=0, seed=3)
    base.update(kw)
    return SimpleNamespace(**base)


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("W,H,S", GEOMETRY)
def test_geometry_is_resize_then_center_crop_of_live_pillow(W, H, S):
    """torchvision's rule written out with Pillow alone (caption_tree.pillow_batch) against captions.geometry + the restated resize: same bytes."""
    from PIL import Image
    from src.datasets import captions as C
    from src.datasets.pil_resize import resize_bicubic
    dst_h, dst_w, y0, x0 = C.geometry(W, H, S)
    assert min(dst_h, dst_w) == S and max(dst_h, dst_w) == int(S * max(W, H) / min(W, H)) and (dst_w if W <= H else dst_h) == S
    assert y0 == int(round((dst_h - S) / 2.0)) and x0 == int(round((dst_w - S) / 2.0)) and y0 + S <= dst_h and x0 + S <= dst_w
    px = np.random.default_rng(W * 1000 + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    im = Image.fromarray(px, "RGB").resize((dst_w, dst_h), Image.BICUBIC).crop((x0, y0, x0 + S, y0 + S))
    assert np.array_equal(np.asarray(im), resize_bicubic(px, dst_h, dst_w, (y0, x0, S, S)))


def test_round_goes_to_even_where_the_difference_is_odd():
    from src.datasets import captions as C
    assert C.geometry(37, 23, 16) == (16, 25, 0, 4)             # (25 - 16) / 2 = 4.5 -> 4
    assert C.geometry(43, 16, 16) == (16, 43, 0, 14)            # 13.5 -> 14
    assert C.geometry(16, 27, 16) == (27, 16, 6, 0)             # 5.5 -> 6
    assert C.geometry(16, 16, 16) == (16, 16, 0, 0)


# ------------------------------------------------------------------------------------------------ uia_resize_batch_rgb's host checks
def test_resize_batch_rgb_host_checks_run_before_anything_is_enqueued():
    """No device here: every refusal returns non-zero from the host checks, names the entry and the image, and leaves the output untouched (host
    memory stands in for the tensors)."""
    from uia_hip import _lib
    lib = _lib.lib()
    B, S = 3, 16
    src = np.zeros(4096, np.uint8)
    out = np.full((B, 3, S, S), 7.0, np.float32)
    need = lib.uia_resize_workspace_bytes(B)
    ws = np.zeros(need + 16, np.uint8)
    wsp = (ws.ctypes.data + 15) & ~15
    good = np.array([[0, 20, 30, 1, S, S, 0, 0], [1200, 9, 8, 3, S, S, 0, 0], [1500, 16, 16, 3, 24, 20, 8, 4]], np.int32)

    def call(desc=good, B=B, S=S, src_p=src.ctypes.data, n=src.size, out_images=out.ctypes.data, ws_bytes=need):
        desc = np.ascontiguousarray(desc, dtype=np.int32)
        return lib.uia_resize_batch_rgb(None, B, S, src_p, n, desc.ctypes.data, wsp, ws_bytes, out_images), lib.uia_last_error().decode()

    def with_(b, col, v):
        d = good.copy()
        d[b, col] = v
        return d

    refusals = [("B = 0", dict(B=0), "B=0"), ("S = 7", dict(S=7), "S=7"), ("2 channels", dict(desc=with_(1, 3, 2)), "image 1 has 2 channels"),
                ("-1 channels (a mask word)", dict(desc=with_(0, 3, -1)), "image 0 has -1 channels"), ("4 channels", dict(desc=with_(2, 3, 4)), "image 2"),
                ("an RGB image leaves the buffer where a gray one would fit", dict(desc=with_(1, 0, 4096 - 9 * 8 * 3 + 1)), "image 1"),
                ("a gray image declared RGB leaves the buffer", dict(desc=np.array([[4096 - 600, 20, 30, 3, S, S, 0, 0]], np.int32), B=1), "image 0"),
                ("window leaves dst", dict(desc=with_(2, 7, 5)), "image 2"), ("dst smaller than the window", dict(desc=with_(0, 4, S - 1)), "image 0"),
                ("a 33x downscale", dict(desc=np.array([[0, 16, 16, 1, S, S, 0, 0], [0, 33 * S, 1, 1, S, S, 0, 0]], np.int32), B=2), "image 1"),
                ("a short workspace", dict(ws_bytes=need - 1), "workspace"), ("null source", dict(src_p=None), "null"),
                ("output inside the source", dict(out_images=src.ctypes.data + 64), "overlap")]
    for what, kw, word in refusals:
        rc, err = call(**kw)
        assert rc != 0 and word in err and "uia_resize_batch_rgb" in err, (what, rc, err)
    assert (out == 7.0).all()


# ------------------------------------------------------------------------------------------------ the csv preparation
def test_preparation_cleans_filters_and_finds_files(tmp_path, caplog):
    import logging
    from src.datasets import captions as C
    expect = T.write_tree(tmp_path)
    with caplog.at_level(logging.WARNING):
        pairs = C.read_pairs(str(tmp_path))
    assert pairs == expect and len(pairs) == T.N_VALID
    assert "Image not_there.png not found in any path during initialization" in caplog.text
    assert pairs[2][0] == T.caption_of(2).replace(" ", "  ", 1)                                     # "§", "™", "é" removed, the ends stripped
    assert pairs[1][1].endswith(os.path.join("medpix_dataset", "images", "pic_01.png"))             # listed with a directory prefix
    assert pairs[3][1].endswith(os.path.join("pmc_curd_dataset", "images", "pic_03.png"))           # a medpix row whose file is in the second folder
    assert C.clean_caption("  5 ± 2 µm (p ≤ 0.05) → ok… «x»\t") == "5 ± 2 µm (p ≤ 0.05) → ok… x"
    assert len("exactly twenty chars") == 20 and all(c != "exactly twenty chars" for c, _ in pairs)


def test_permutation_is_pandas_sample_and_the_cut_is_90_10(tmp_path):
    from src.datasets import captions as C
    assert C.permutation(10, 3) == [5, 4, 1, 2, 9, 6, 7, 0, 3, 8]         # what pandas 2.3.3 df.sample(frac=1, random_state=3) draws for 10 rows
    pairs = T.write_tree(tmp_path)
    train, val = C.split_pairs(pairs, 3)
    order = C.permutation(24, 3)
    assert len(train) == 21 and len(val) == 3 and train + val == [pairs[i] for i in order]


def test_one_dataset_absent_and_both_absent(tmp_path):
    from src.datasets import captions as C
    expect = T.write_tree(tmp_path / "a", datasets=("pmc_curd_dataset",))
    assert C.read_pairs(str(tmp_path / "a")) == expect and len(expect) == 10
    expect = T.write_tree(tmp_path / "b", datasets=("medpix_dataset",))
    assert C.read_pairs(str(tmp_path / "b")) == expect and len(expect) == 14
    os.makedirs(tmp_path / "c")
    with pytest.raises(RuntimeError, match="neither"):
        C.read_pairs(str(tmp_path / "c"))


def test_precedence_of_the_data_flags_and_data_root_still_refused(tmp_path):
    from src.datasets import captions as C
    from src.models import contrastive
    from src.models.biomedclip import finetune
    assert C.chosen(_args("x")) and not C.chosen(_args("x", synthetic=True)) and not C.chosen(_args("x", data_pt="f.pt")) and not C.chosen(_args(None))
    a = finetune.get_args(["--finetune_root", "d", "--tokenizer_json", "t.json"])
    assert a.finetune_root == "d" and a.tokenizer_json == "t.json" and C.chosen(a)
    with pytest.raises(RuntimeError, match="contrastive.*--finetune_root"):
        contrastive.run(_args("x", data_root=str(tmp_path)), None, None, None)


# ------------------------------------------------------------------------------------------------ the ring of byte slots
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("captions")
    T.write_tree(root)
    return str(root), T.write_tokenizer(root / "tok.json")


@pytest.mark.parametrize("workers", [0, 2])
@pytest.mark.parametrize("check", ["slot", "abandon"])
def test_ring_with_and_without_workers(tree, check, workers):
    """tests/caption_ring_driver.py: `slot` — a worker's slot holds what pack_ragged-style packing gives; `abandon` — more abandoned iterations than
    there are slots, and every slot is back.  Worker processes are forked, so that case runs in a fresh process that never opens the GPU."""
    import subprocess
    import caption_ring_driver as D
    if workers == 0:
        getattr(D, check)(tree[0], tree[1], 0)
        return
    r = subprocess.run([sys.executable, os.path.join(HERE, "caption_ring_driver.py"), check, tree[0], tree[1], str(workers)], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert r.returncode == 0 and "ring ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_an_oversized_image_arrives_resized_by_pillow(tree, tmp_path):
    """Above the byte limit (the 1100 x 1000 file) and beyond a 32x downscale (S = 8 from 300 x 280): the worker ships Pillow's resize, the descriptor
    keeps the size (an identity resize) and carries the window."""
    from PIL import Image
    from src.datasets import captions as C
    big = os.path.join(tree[0], "medpix_dataset", "images", T.BIG)
    px, geom, _ = C.CaptionPairs([("c", big)], 32)[0]
    assert 1100 * 1000 > C.image_limit(32) and geom == C.geometry(1100, 1000, 32) == (32, 35, 0, 2) and px.shape == (32, 35)
    assert np.array_equal(px, np.asarray(Image.open(big).resize((35, 32), Image.BICUBIC)))
    path = str(tmp_path / "steep.png")
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (280, 300, 3), dtype=np.uint8), "RGB").save(path)
    px, geom, _ = C.CaptionPairs([("c", path)], 8)[0]
    assert geom == (8, 8, 0, 0) and px.shape == (8, 8, 3) and 280 / 8 > 32
    assert np.array_equal(px, np.asarray(Image.open(path).resize((8, 8), Image.BICUBIC)))
    ring = C.ByteSlotRing(1, 1, C.image_limit(8), 0, None)
    _, slot, B, nbytes, _ = ring([(px, geom, "c")])
    assert ring.desc[slot, 0].tolist() == [0, 8, 8, 3, 8, 8, 0, 0] and nbytes == 192
    # a long strip: resized it is still above the limit, so the worker cuts it to its window
    strip = np.zeros((60, 30000, 3), np.uint8)
    strip[:, 14000:16000] = np.random.default_rng(1).integers(0, 256, (60, 2000, 3), dtype=np.uint8)
    Image.fromarray(strip, "RGB").save(path)
    px, geom, _ = C.CaptionPairs([("c", path)], 32)[0]
    assert 32 * 16000 * 3 > C.image_limit(32) and geom == (32, 32, 0, 0) and px.shape == (32, 32, 3)
    assert np.array_equal(px, np.asarray(Image.open(path).resize((16000, 32), Image.BICUBIC).crop((7984, 0, 8016, 32))))


# ------------------------------------------------------------------------------------------------ --tokenizer_json
def test_tokenizer_file_ids_truncation_and_padding(tmp_path):
    from src.utils.tokenizer_file import FileTokenizer
    tk = FileTokenizer(T.write_tokenizer(tmp_path / "t.json"), 6)
    ids = tk(["lesion scan of", "mass shows the liver of scan lesion", "unknown liver"])
    assert ids.dtype == torch.long and ids.tolist() == [[2, 3, 4, 5, 10, 0],                       # [CLS] .. [SEP], padded with id 0 to the context length
                                                        [2, 9, 8, 6, 7, 10],                       # cut to 6: [SEP] is kept
                                                        [2, 1, 7, 10, 0, 0]]                       # [UNK]
    assert tk("scan").shape == (1, 6) and tk.largest_id() == 10
    tk.check(11, pools_at_argmax=True)


def test_tokenizer_file_refusals(tmp_path):
    from src.models.biomedclip import finetune as biomed
    from src.models.clip import finetune as clip
    from src.utils.tokenizer_file import FileTokenizer
    good, bert = T.write_tokenizer(tmp_path / "t.json"), T.write_tokenizer(tmp_path / "b.json", sep_largest=False)
    with pytest.raises(RuntimeError, match="embedding table has 10 rows"):
        FileTokenizer(good, 6).check(10, pools_at_argmax=False)
    with pytest.raises(RuntimeError, match="arg-max"):
        FileTokenizer(bert, 6).check(11, pools_at_argmax=True)
    FileTokenizer(bert, 6).check(11, pools_at_argmax=False)
    # through the families' make_tokenizer, which runs before anything is launched
    toy = "(64, 32, 2, 128, 8, 16, 4000, 128, 2, 2)"
    assert clip.make_tokenizer(clip.get_args(["--model_config", toy, "--tokenizer_json", good]))(["scan"]).shape == (1, 16)
    with pytest.raises(RuntimeError, match="arg-max"):
        clip.make_tokenizer(clip.get_args(["--model_config", toy, "--tokenizer_json", bert]))
    with pytest.raises(RuntimeError, match="embedding table has 8 rows"):
        clip.make_tokenizer(clip.get_args(["--model_config", "(64, 32, 2, 128, 8, 16, 8, 128, 2, 2)", "--tokenizer_json", good]))
    small = ("dict(embed_dim=128, vision_cfg=dict(img_size=32, patch_size=8, embed_dim=128, depth=2, num_heads=2), text_cfg=dict(vocab_size=9, "
             "hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64))")
    with pytest.raises(RuntimeError, match="embedding table has 9 rows"):
        biomed.make_tokenizer(biomed.get_args(["--model_config", small, "--tokenizer_json", bert]))
    assert type(biomed.make_tokenizer(biomed.get_args([]))).__name__ == "SyntheticTokenizer"      # without the flag the stand-in stays
