"""-m gpu: the --finetune_root path end to end on a generated tree (tests/caption_tree.py: "L", "RGB", "P", "RGBA" and JPEG files, one above the
per-image byte limit).  Loader workers are forked before a process opens the GPU, so every case is a fresh child process
(tests/caption_gpu_driver.py): the loader, prefetcher and stage against Pillow's Image.open -> convert("RGB") -> resize -> crop -> / 255, bit for
bit, with 0 and with 2 workers and a last partial batch; and one fine-tune entry per text-tower layout, with real ids from a tokenizer file."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import caption_tree as T  # noqa: E402

pytest.importorskip("PIL")
DRIVER = os.path.join(HERE, "caption_gpu_driver.py")
BIOMED_TOY = ("dict(embed_dim=128, vision_cfg=dict(img_size=32, patch_size=8, embed_dim=128, depth=2, num_heads=2), "
              "text_cfg=dict(vocab_size=30000, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64))")
CLIP_TOY = "(64, 32, 2, 128, 8, 16, 4000, 128, 2, 2)"
ENTRIES = {"biomedclip": ["--model_config", BIOMED_TOY, "--method", "mona", "--accumulation_steps", "1"], "clip": ["--model_config", CLIP_TOY, "--ckpt", ""]}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("captions_gpu")
    T.write_tree(root)
    return str(root), T.write_tokenizer(root / "tok.json")


def _child(argv, cwd):
    r = subprocess.run([sys.executable, DRIVER] + argv, capture_output=True, text=True, timeout=300, cwd=str(cwd))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("workers", [0, 2])
def test_loader_prefetcher_and_stage_equal_pillow_bit_for_bit(tree, workers, tmp_path):
    assert "loader ok" in _child(["loader", tree[0], tree[1], str(workers)], tmp_path)


@pytest.mark.parametrize("family", list(ENTRIES))
def test_entry_point_trains_from_the_folders_with_real_token_ids(tree, family, tmp_path):
    """24 pairs: 21 train (two batches of 8, drop_last) and 3 validation (one partial batch); two epochs."""
    out = _child(["entry", family, "--finetune_root", tree[0], "--tokenizer_json", tree[1], "--img_size", "32", "--batch_size", "8", "--epochs", "2",
                  "--num_workers", "2", "--lr", "1e-3", "--dtype", "bf16", "--exp", "ft"] + ENTRIES[family], tmp_path)
    res = json.loads([line for line in out.splitlines() if line.startswith("RESULT ")][-1][len("RESULT "):])
    assert len(res["epochs"]) == 2 and all("loader_wait_ms" in e and e["loader_wait_ms"] >= 0.0 and e["batches"] == 2 for e in res["epochs"])
    assert torch.isfinite(torch.tensor([res["best_val"], res["last_train"]])).all() and res["best_val"] > 0.0 and res["last_train"] > 0.0
    log = open(tmp_path / "runs" / "ft" / "log.log").read()
    assert "Train samples: 21, Val samples: 3" in log and "stand-in tokenizer" not in log
    state = torch.load(tmp_path / "runs" / "ft" / "best_model.pth", map_location="cpu")
    assert state and all("mona" in k.lower() for k in state) and all(bool(torch.isfinite(v).all()) for v in state.values())
