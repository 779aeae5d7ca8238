"""-m gpu: uia_augment_gather (csrc/augment.hip) against uia_augment_batch on the gathered rows, bit for bit (that kernel is pinned to Pillow by
tests/golden/augment_cases.npz in tests/test_augment_*.py and is not under test here), for fp32 and uint8 resident sets at sizes whose rows start on
16, 4 and odd bytes; the Pillow fixtures through the gather form; the refusals; an epoch of the resident set; and the four few-shot entries end to end."""
import csv
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import augment_reference as R  # noqa: E402
from guarded_out import dev  # noqa: E402

GUARD = 64
SRC = [0, 4, 4, 2, 1, 0, 3]                                     # N = 5 resident rows, B = 7 outputs: repeats, and B > N


class Guarded:
    """A device tensor GUARD elements inside a sentinel-filled buffer."""

    def __init__(self, shape, dtype):
        self.n = math.prod(shape)
        self.sentinel = float("nan") if dtype == torch.float32 else 0xA5
        self.buf = torch.full((GUARD + self.n + GUARD,), self.sentinel, dtype=dtype, device=dev())
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)

    def untouched(self, whole=False):
        b = self.buf.cpu()
        parts = [b] if whole else [b[:GUARD], b[GUARD + self.n:]]
        return all(bool(torch.isnan(p).all()) if self.sentinel != self.sentinel else bool((p == self.sentinel).all()) for p in parts)


def programs(S, with_mask):
    """Seven programs over every opcode: one empty, one of 13 ops with two crops; the src column holds SRC."""
    lo = int(np.ceil(np.sqrt(0.8) * S))
    t = R.make_table([
        [],
        [(R.AUTOCONTRAST, 0, 0, 0), (R.EQUALIZE, 0, 0, 0), (R.BLUR, 1.0, 0, 0), (R.CONTRAST, 1.2, 0, 0), (R.BRIGHTNESS, 0.9, 0, 0), (R.SHARPNESS, 1.1, 0, 0),
         (R.POSTERIZE, 5, 0, 0), (R.SOLARIZE, 200, 0, 0), (R.IDENTITY, 0, 0, 0), (R.CROP, 1, 0, S - 1), (R.HFLIP, 0, 0, 0), (R.VFLIP, 0, 0, 0), (R.CROP, 0, 1, S - 2)],
        [(R.BLUR, 0.8, 0, 0), (R.SHARPNESS, 0.8, 0, 0)],
        [(R.CONTRAST, 0.75, 0, 0), (R.SOLARIZE, 100, 0, 0), (R.HFLIP, 0, 0, 0)],
        [(R.EQUALIZE, 0, 0, 0), (R.VFLIP, 0, 0, 0), (R.CROP, S - lo, S - lo, lo)],
        [(R.POSTERIZE, 3, 0, 0), (R.AUTOCONTRAST, 0, 0, 0)],
        [(R.BRIGHTNESS, 1.25, 0, 0), (R.IDENTITY, 0, 0, 0)]], with_mask=with_mask)
    assert t[0, 0, 0] == 0 and t[1, 0, 0] == 13 and set(t[:, 1:, 0].reshape(-1).tolist()) == set(range(12))
    t[:, 0, 2] = SRC
    return torch.from_numpy(t)


@pytest.mark.parametrize("S", [8, 9, 10, 33])
@pytest.mark.parametrize("source", ["uint8", "fp32"])
@pytest.mark.parametrize("with_mask", [True, False])
def test_gather_equals_the_batch_kernel_on_the_gathered_rows(S, source, with_mask):
    from uia_hip import ops
    g = torch.Generator().manual_seed(100 * S + with_mask)
    N = 5
    if source == "uint8":
        resident = torch.randint(0, 256, (N, 1, S, S), generator=g, dtype=torch.uint8)
        resident[3] = 77                                        # a flat row: autocontrast / equalize take their identity branches
        rows = resident[SRC].float() / 255
    else:
        resident = torch.rand(N, 1, S, S, generator=g)         # off the 8-bit grid: quantised once by both kernels
        rows = resident[SRC]
    masks = torch.randint(0, 256, (N, 1, S, S), generator=g, dtype=torch.uint8) if with_mask else None
    table = programs(S, with_mask)
    res_d, masks_d = resident.to(dev()), None if masks is None else masks.to(dev())
    oi, om = Guarded((7, 1, S, S), torch.float32), Guarded((7, 1, S, S), torch.uint8) if with_mask else None
    ops.augment_gather(res_d, masks_d, table, oi.t, None if om is None else om.t)
    want_i, want_m = ops.augment_batch(rows.contiguous().to(dev()), None if masks is None else masks[SRC].contiguous().to(dev()), table)
    torch.cuda.synchronize()
    assert oi.untouched() and (om is None or om.untouched()), "a write outside the outputs"
    got, want = oi.t.cpu().numpy().view(np.int32), want_i.cpu().numpy().view(np.int32)
    for b in range(7):
        assert np.array_equal(got[b], want[b]), f"S={S} {source}: output {b} (row {SRC[b]}, {int(table[b, 0, 0])} ops): {(got[b] != want[b]).sum()} pixels differ"
    if with_mask:
        assert torch.equal(om.t.cpu(), want_m.cpu())
    # the same call twice: deterministic
    again_i, again_m = ops.augment_gather(res_d, masks_d, table)
    assert np.array_equal(again_i.cpu().numpy().view(np.int32), got) and (not with_mask or torch.equal(again_m.cpu(), om.t.cpu()))


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(HERE, "golden", "augment_cases.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("S", [37, 64])
def test_pillow_cases_through_the_gather_form_in_shuffled_order(S):
    """The rule of tests/test_augment_host.py for these fixtures: every op but the blur, alone and composed, equals Pillow's stored result pixel for
    pixel, image and mask (the blur is this build's own Gaussian and is held to its float64 value elsewhere).  Here the three source planes are the
    resident set, as bytes, and the 49 cases are the outputs, in shuffled order."""
    from uia_hip import ops
    z = golden()
    names = [str(n) for n in z[f"name_{S}"]]
    order = np.random.default_rng(S).permutation(len(names))
    table = z[f"tab_{S}"][order].copy()
    table[:, 0, 1] = 1
    table[:, 0, 2] = z[f"src_{S}"][order]
    resident = torch.from_numpy(z[f"in_{S}"][:, None].copy()).to(dev())
    masks = torch.from_numpy(z[f"mask_{S}"][:, None].copy()).to(dev())
    oi, om = ops.augment_gather(resident, masks, torch.from_numpy(np.ascontiguousarray(table)))
    oi, om = oi.cpu().numpy()[:, 0], om.cpu().numpy()[:, 0]
    checked = 0
    for b, c in enumerate(order):
        if names[c].startswith("blur"):
            continue
        want = z[f"out_{S}"][c].astype(np.float32) / np.float32(255)
        assert np.array_equal(oi[b].view(np.int32), want.view(np.int32)), (names[c], int((oi[b] != want).sum()))
        assert np.array_equal(om[b], z[f"outmask_{S}"][c]), names[c]
        checked += 1
    assert checked >= 40


def test_gather_refusals_return_non_zero_and_leave_the_outputs_untouched():
    from uia_hip import _lib, ops
    lib = _lib.lib()
    N, B, S = 5, 7, 9
    resident = torch.randint(0, 256, (N, 1, S, S), dtype=torch.uint8).to(dev())
    masks = torch.randint(0, 2, (N, 1, S, S), dtype=torch.uint8).to(dev())
    big = torch.zeros(4 * B * S * S + 64, dtype=torch.uint8, device=dev())          # a resident set an fp32 output of B rows fits inside
    oi, om = Guarded((B, 1, S, S), torch.float32), Guarded((B, 1, S, S), torch.uint8)
    ws = ops.augment_workspace(B, S, dev())
    good = programs(S, True).numpy()
    st = torch.cuda.current_stream().cuda_stream

    def call(tab=good, N=N, dt=1, images=resident.data_ptr(), masks=masks.data_ptr(), out_images=oi.t.data_ptr(), out_masks=om.t.data_ptr()):
        tab = np.ascontiguousarray(tab, dtype=np.int32)
        return lib.uia_augment_gather(st, N, B, S, dt, images, masks, tab.ctypes.data, ws.data_ptr(), ws.numel(), out_images, out_masks)

    def with_src(v):
        t = good.copy()
        t[5, 0, 2] = v
        return t

    for what, kw in [("src = N", dict(tab=with_src(N))), ("src = -1", dict(tab=with_src(-1))), ("src_dtype = 2", dict(dt=2)), ("N = 0", dict(N=0))]:
        assert call(**kw) != 0, what
        assert b"uia_augment_gather" in lib.uia_last_error()
    torch.cuda.synchronize()
    assert oi.untouched(whole=True) and om.untouched(whole=True)
    # an output that overlaps the resident set: the set is `big` (N' rows of bytes), the fp32 output lies inside it; pre-filled with a sentinel
    big.fill_(0x5A)
    n_big = big.numel() // (S * S)
    assert call(N=n_big, images=big.data_ptr(), out_images=big.data_ptr() + 16) != 0 and b"overlap" in lib.uia_last_error()
    assert call(out_masks=masks.data_ptr() + (N - 1) * S * S) != 0 and b"overlap" in lib.uia_last_error()
    torch.cuda.synchronize()
    assert bool((big == 0x5A).all()) and oi.untouched(whole=True) and om.untouched(whole=True)
    assert call() == 0                                              # and the same buffers take a good table
    torch.cuda.synchronize()
    # rows.float() / 255 is the loaders' host division (IEEE); on the device torch multiplies by a rounded 1 / 255, which is one ulp off for some bytes
    want_i, want_m = ops.augment_batch((resident.cpu()[SRC].float() / 255).contiguous().to(dev()), masks[SRC].contiguous(), torch.from_numpy(good))
    assert torch.equal(oi.t, want_i) and torch.equal(om.t, want_m)
    with pytest.raises(_lib.UiaError):
        ops.augment_gather(resident.cpu(), None, torch.from_numpy(good))
    with pytest.raises(_lib.UiaError):
        ops.augment_gather(resident.to(torch.int16), None, torch.from_numpy(good))


@pytest.mark.parametrize("kind", ["segmentation", "classification"])
def test_resident_epoch_with_the_stage_off_is_a_permutation_of_the_uploaded_rows(kind):
    from src.datasets.resident import ResidentTrainSet
    n, S = 5, 12
    g = torch.Generator().manual_seed(4)
    images = torch.randint(0, 256, (n, 1, S, S), generator=g, dtype=torch.uint8)
    second = torch.randint(0, 2, (n, 1, S, S), generator=g, dtype=torch.uint8) if kind == "segmentation" else torch.tensor([3, 1, 4, 1, 5])
    rs = ResidentTrainSet(images, second, 5, seed=11, device=dev())
    rs.set_epoch(1)
    batches = [(im.clone(), lab.clone(), ready) for im, lab, ready in rs]
    assert len(batches) == 1 and rs.augmented == 0
    im, lab, ready = batches[0]
    ready.synchronize()
    im, lab = im.cpu(), lab.cpu()
    want = images.float() / 255
    rows = [next(r for r in range(n) if np.array_equal(im[b].numpy().view(np.int32), want[r].numpy().view(np.int32))) for b in range(n)]
    assert sorted(rows) == list(range(n))
    assert torch.equal(lab, second[rows])


# ------------------------------------------------------------------------------------------------ the four entries
FPN_CFG = dict(embed_dim=64, vision_cfg=dict(img_size=32, patch_size=8, embed_dim=768, depth=3, num_heads=12, mlp_ratio=0.25),
               text_cfg=dict(vocab_size=64, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64, max_position_embeddings=16))
TOY = ["--synthetic", "--img_size", "32", "--patch_size", "8", "--reduce_dim", "64", "--batch_size", "8", "--synthetic_train", "48",
       "--synthetic_val", "16", "--synthetic_test", "16", "--device", "cuda:0", "--dtype", "fp32"]                    # tests/test_classification_gpu.py's
BIOMED = TOY + ["--model_config", repr(FPN_CFG), "--extract_layers", "0,1,2", "--num_workers", "0"]
BASELINE = ["--synthetic", "--synthetic_train", "8", "--synthetic_val", "4", "--synthetic_test", "4", "--img_size", "64", "--batch_size", "4", "--num_workers", "0",
            "--device", "cuda:0"]
ENTRIES = {
    "biomedclip_cls": ("src.models.biomedclip.fewshot_classification", BIOMED + ["--shots_per_class", "1"], 2, 48, "fewshot_cls"),
    "biomedclip_seg": ("src.models.biomedclip.fewshot_segmentation", BIOMED + ["--synthetic_train", "64", "--train_ratio", "0.02", "--no-viz"], 1, 64, "fewshot_seg"),
    "resnet_cls": ("src.models.baselines.fewshot_classification", BASELINE + ["--shots_per_class", "1"], 2, 8, "fewshot_resnet_cls"),
    "unet_seg": ("src.models.baselines.fewshot_segmentation", BASELINE + ["--train_ratio", "0.25", "--no-viz"], 2, 8, "fewshot_unet_seg"),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_fewshot_entry_trains_checkpoints_and_tests(entry, tmp_path, monkeypatch, capsys):
    import importlib
    import json
    module, argv, n, total, exp = ENTRIES[entry]
    cli = importlib.import_module(module)
    monkeypatch.chdir(tmp_path)
    argv = argv + ["--epochs", "2", "--val_every", "1", "--dataset", "SYN", "--stats_json", "stats.json"]
    out = cli.main(argv)
    printed = capsys.readouterr().out
    assert f"    - Original training samples: {total}\n    - Sampled training samples: {n}\n" in printed
    assert (out["sampled_train_count"], out["original_train_count"]) == (n, total) and out["iters"] == 2 and out["augmented_images"] == 0
    assert [e["updates"] for e in out["epochs"]] == [1, 1]
    stats = json.load(open("stats.json"))
    assert (stats["sampled_train_count"], stats["original_train_count"]) == (n, total)
    train_dir = f"runs/{exp}/SYN/train"
    assert os.path.exists(f"{train_dir}/best_model.pth") and os.path.exists(out["test"]["results_csv"])
    assert f"Training samples: {n} / {total}" in open(f"{train_dir}/log.log").read()
    rows = [json.loads(line) for line in open(f"{train_dir}/log/scalars.jsonl")]
    losses = [r["value"] for r in rows if r["tag"].endswith("_loss")]
    assert losses and all(math.isfinite(v) for v in losses) and math.isfinite(out["last_loss"]) and math.isfinite(out["test"]["loss"])
    if entry.endswith("cls"):
        assert len(out["val"]) == 1                                     # validations follow epochs 1, 2, ... (`epoch > 0`)
        files = sorted(os.listdir(f"{train_dir}/roc_curves"))
        assert files == [f"roc_curve_iter_{out['iters']}.csv"]
        table = list(csv.reader(open(f"{train_dir}/roc_curves/{files[0]}")))
        assert table[0] == ["fpr", "tpr", "threshold"] and len(table) >= 3
        pts = [[float(v) for v in r] for r in table[1:]]
        assert pts[0][:2] == [0.0, 0.0] and pts[-1][:2] == [1.0, 1.0] and all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(pts, pts[1:]))
    else:
        assert not os.path.exists(f"{train_dir}/roc_curves")
    # --test afterwards reads the checkpoint and evaluates the whole test split: the figures of the run's own closing test pass
    again = cli.main(argv + ["--test"])["test"]
    key = "acc" if entry.endswith("cls") else "dice_mean"
    print(f"{entry}: test loss {out['test']['loss']!r} / {again['loss']!r}, {key} {out['test'][key]!r} / {again[key]!r}")
    assert abs(again["loss"] - out["test"]["loss"]) <= 1e-6 and abs(again[key] - out["test"][key]) <= 1e-6


def test_unet_fewshot_runs_at_one_training_image(tmp_path, monkeypatch):
    """DESIGN.md §4 "Few-shot": B = 1 runs on the BatchNorm baselines (the statistics are over B H W values per channel)."""
    from src.models.baselines import fewshot_segmentation as cli
    monkeypatch.chdir(tmp_path)
    out = cli.main(BASELINE + ["--train_ratio", "0.125", "--no-viz", "--epochs", "2", "--val_every", "1", "--dataset", "SYN"])
    assert out["sampled_train_count"] == 1 and out["iters"] == 2 and math.isfinite(out["last_loss"]) and math.isfinite(out["test"]["loss"])


def test_fewshot_segmentation_on_a_uint8_file_runs_the_stage_in_the_forming_launch(tmp_path, monkeypatch):
    """--data_pt rows stay bytes on the device and the default --strong_augs / --weak_augs run inside the launch that forms the batch; with both off the
    same entry counts no augmented image."""
    from src.models.biomedclip import fewshot_segmentation as cli
    monkeypatch.chdir(tmp_path)
    S, n = 32, 24
    g = torch.Generator().manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    cx = torch.randint(S // 4, 3 * S // 4, (n,), generator=g)
    labels = (((yy[None] - S // 2) ** 2 + (xx[None] - cx[:, None, None]) ** 2) <= (S // 5) ** 2)[:, None].to(torch.uint8) * 255
    images = (torch.randint(0, 120, (n, 1, S, S), generator=g) + labels // 2).to(torch.uint8)
    torch.save({"images": images, "labels": labels, "split": {"train": list(range(16)), "val": list(range(16, 20)), "test": list(range(20, 24))}}, "seg.pt")
    argv = [a for a in BIOMED if a != "--synthetic"] + ["--data_pt", "seg.pt", "--batch_size", "4", "--train_ratio", "0.5", "--epochs", "3", "--val_every", "5",
                                                        "--no-viz", "--dataset", "PT"]
    on = cli.main(argv)
    assert (on["sampled_train_count"], on["original_train_count"], on["iters"]) == (8, 16, 6) and 0 < on["augmented_images"] <= 24
    assert math.isfinite(on["last_loss"]) and math.isfinite(on["test"]["loss"])
    off = cli.main(argv + ["--no-strong_augs", "--no-weak_augs", "--exp", "off"])
    assert off["augmented_images"] == 0 and off["iters"] == 6 and math.isfinite(off["test"]["loss"])
