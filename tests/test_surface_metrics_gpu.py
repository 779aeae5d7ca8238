"""-m gpu: the HD95 / ASD kernel (`uia_surface_distances`, csrc/surface.hip) against the float64 restatement of tests/surface_reference.py, its
determinism, MetricAccumulator on device tensors (statistics, no host sync in update()), and the CLIPSeg entry point's test() with real HD95 / ASD."""
import math
import os
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import surface_reference as R  # noqa: E402


def dev():
    return torch.device("cuda:0")


def _blobs(B, H, W, seed, k=3):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    out = torch.zeros(B, H, W, dtype=torch.bool)
    for b in range(B):
        for _ in range(k):
            cy, cx = float(torch.rand(1, generator=g)) * H, float(torch.rand(1, generator=g)) * W
            ry, rx = 1 + float(torch.rand(1, generator=g)) * H / 4, 1 + float(torch.rand(1, generator=g)) * W / 4
            out[b] |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    return out


def _logits_of(mask, seed, scale=2.0):
    """logits [B,2,H,W] with arg-max == mask, random margins."""
    g = torch.Generator().manual_seed(seed)
    l0 = torch.randn(mask.shape, generator=g) * scale
    gap = torch.rand(mask.shape, generator=g) * scale + 1e-3
    l1 = torch.where(mask, l0 + gap, l0 - gap)
    return torch.stack([l0, l1], 1)


def _case(name):
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    if name.startswith("blobs"):
        H, W = {"blobs64": (64, 64), "blobs224": (224, 224), "blobs96x160": (96, 160)}[name]
        B = 8 if H < 224 else 4
        return _logits_of(_blobs(B, H, W, 1), 2), _blobs(B, H, W, 3).float()[:, None]
    if name in ("h1", "w1"):
        shape = (6, 1, 77) if name == "h1" else (6, 77, 1)
        p, gt = torch.rand(shape, generator=g) > 0.6, torch.rand(shape, generator=g) > 0.8
        p[0] = True
        gt[1] = True
        p[2] = False
        return _logits_of(p, 4), gt.float()[:, None]
    if name == "borders":
        p, gt = _blobs(6, 48, 48, 5, k=8), torch.ones(6, 48, 48, dtype=torch.bool)
        gt[1, 10:30, 12:20] = False
        gt[2] = _blobs(1, 48, 48, 6, k=8)[0]
        p[3] = True                                              # full against full
        p[4] = False                                             # empty P
        gt[5] = False                                            # empty G
        p[0, :, 0] = p[0, 0, :] = p[0, :, -1] = p[0, -1, :] = True
        lab = gt.float()[:, None]
        logits = _logits_of(p, 7)
        extra_l = _logits_of(torch.zeros(1, 48, 48, dtype=torch.bool), 8)          # both empty
        return torch.cat([logits, extra_l]), torch.cat([lab, torch.zeros(1, 1, 48, 48)])
    if name == "ties_nan":
        B, H, W = 6, 40, 40
        l = torch.randint(-2, 3, (B, 2, H, W), generator=g).float()         # many exact ties -> class 0
        nanm = torch.rand(B, 2, H, W, generator=g) < 0.15
        l[nanm] = float("nan")
        return l, (torch.rand(B, 1, H, W, generator=g) > 0.5).float() * torch.where(torch.rand(B, 1, H, W, generator=g) > 0.5, 1.0, 0.3)
    if name == "checker64":
        yy, xx = torch.meshgrid(torch.arange(64), torch.arange(64), indexing="ij")
        cb = ((yy + xx) % 2 == 0)[None].repeat(4, 1, 1)
        cb[1] = ~cb[1]
        gt = torch.stack([cb[0], ~cb[0], _blobs(1, 64, 64, 9)[0], torch.rand(64, 64, generator=g) > 0.5])
        return _logits_of(cb, 10), gt.float()[:, None]
    if name == "noise64":
        return torch.randn(8, 2, 64, 64, generator=g), torch.where(torch.rand(8, 1, 64, 64, generator=g) > 0.5, 1.0, 0.0)
    if name == "noise224":
        lab = _blobs(3, 224, 224, 11).float()[:, None]
        lab[2] = (torch.rand(1, 224, 224, generator=g) > 0.5).float()
        return torch.randn(3, 2, 224, 224, generator=g), lab
    raise KeyError(name)


def _check(hd, asd, logits, label, percentile):
    want_hd, want_asd = R.surface_distances(logits, label, percentile)
    hd, asd = hd.cpu().numpy(), asd.cpu().numpy()
    assert np.array_equal(np.isfinite(hd), np.isfinite(want_hd)), (hd, want_hd)
    assert np.array_equal(np.isfinite(asd), np.isfinite(want_asd)), (asd, want_asd)
    f = np.isfinite(want_hd)
    assert np.all(np.abs(hd[f] - want_hd[f]) <= 2e-6 * np.maximum(1.0, np.abs(want_hd[f]))), (hd[f], want_hd[f])
    assert np.all(np.abs(asd[f] - want_asd[f]) <= 1e-6 * np.abs(want_asd[f]) + 1e-12), (asd[f], want_asd[f])
    return f


CASES = ["blobs64", "blobs224", "blobs96x160", "h1", "w1", "borders", "ties_nan", "checker64", "noise64", "noise224"]


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_restatement(name):
    from uia_hip import ops
    logits, label = _case(name)
    hd, asd = ops.surface_distances(logits.to(dev()), label.to(dev()), 95.0)
    assert hd.dtype == torch.float64 and asd.dtype == torch.float64 and tuple(hd.shape) == (logits.shape[0],)
    f = _check(hd, asd, logits, label, 95.0)
    if name.startswith("blobs") or name == "noise224":
        assert f.all()
    if name == "borders":
        assert list(f) == [True, True, True, True, False, False, False]
        assert float(hd[3]) == 0.0 and float(asd[3]) == 0.0


@pytest.mark.parametrize("name", ["blobs64", "noise64", "borders", "ties_nan", "h1"])
@pytest.mark.parametrize("percentile", [0.0, 50.0, 95.0, 100.0])
def test_kernel_percentiles(name, percentile):
    from uia_hip import ops
    logits, label = _case(name)
    hd, asd = ops.surface_distances(logits.to(dev()), label.to(dev()), percentile)
    _check(hd, asd, logits, label, percentile)


def test_percentile_zero_is_the_maximum_and_hundred_too():
    from uia_hip import ops
    logits, label = _case("blobs64")
    a, _ = ops.surface_distances(logits.to(dev()), label.to(dev()), 0.0)
    b, _ = ops.surface_distances(logits.to(dev()), label.to(dev()), 100.0)
    c, _ = ops.surface_distances(logits.to(dev()), label.to(dev()), 95.0)
    assert torch.equal(a, b) and bool((c <= a).all())


def test_bf16_logits_are_converted():
    from src.losses.dice import surface_distances_per_image
    logits, label = _case("blobs64")
    lb = logits.to(dev()).bfloat16()
    hd, asd = surface_distances_per_image(lb, label.to(dev()))
    _check(hd, asd, lb.float().cpu(), label, 95.0)


def test_two_calls_agree_bit_for_bit_at_128_images_of_224():
    from uia_hip import ops
    g = torch.Generator().manual_seed(21)
    m = _blobs(128, 224, 224, 12, k=2)
    logits = _logits_of(m, 13)
    logits[64:80] = torch.randn(16, 2, 224, 224, generator=g)              # noise images
    label = _blobs(128, 224, 224, 14, k=2).float()[:, None]
    label[100] = 0
    logits, label = logits.to(dev()), label.to(dev())
    h1, a1 = ops.surface_distances(logits, label)
    h2, a2 = ops.surface_distances(logits, label)
    assert torch.equal(h1.view(torch.int64), h2.view(torch.int64)) and torch.equal(a1.view(torch.int64), a2.view(torch.int64))
    assert not bool(torch.isfinite(h1[100])) and int(torch.isfinite(h1).sum()) >= 120
    idx = [0, 70, 100, 127]
    _check(h1[idx], a1[idx], logits[idx].cpu(), label[idx].cpu(), 95.0)


def _crit(p, y):
    return (p[:, 1] - y[:, 0]).abs().mean()


def test_metric_accumulator_reports_hd95_and_asd_from_device_tensors():
    from src.utils.tools import MetricAccumulator
    batches = [_case("blobs64"), _case("borders")]
    acc, host = MetricAccumulator(type="seg", criterion=_crit, num_classes=2), MetricAccumulator(type="seg", criterion=_crit, num_classes=2)
    hd, asd = [], []
    for logits, label in batches:
        acc.update(logits.to(dev()), label.to(dev()))
        host.update(logits, label)
        h, a = R.surface_distances(logits, label, 95.0)
        hd += list(h)
        asd += list(a)
    s, c = acc.compute(), host.compute()
    for key, vals in (("hd95", hd), ("asd", asd)):
        m, sd = R.finite_stats(vals)
        assert s[f"{key}_mean"] == pytest.approx(m, rel=1e-6) and s[f"{key}_std"] == pytest.approx(sd, rel=1e-6), (key, s)
    for k in ("dice_mean", "dice_std", "iou_mean", "iou_std"):
        assert s[k] == pytest.approx(c[k], rel=1e-12), k
    assert s["loss"] == pytest.approx(c["loss"], rel=1e-6)
    assert all(math.isnan(c[k]) for k in ("hd95_mean", "hd95_std", "asd_mean", "asd_std"))        # CPU tensors: unchanged
    three = MetricAccumulator(type="seg", criterion=lambda p, y: p.mean(), num_classes=3)
    three.update(torch.randn(2, 3, 16, 16, device=dev()), torch.randint(0, 3, (2, 1, 16, 16), device=dev()).float())
    assert math.isnan(three.compute()["hd95_mean"])
    acc.reset()
    assert math.isnan(acc.compute()["hd95_mean"])


def test_update_does_not_synchronise_with_the_host():
    from src.losses.dice import DiceCELoss
    from src.utils.tools import MetricAccumulator
    logits, label = _case("blobs64")
    logits, label = logits.to(dev()), label.to(dev())
    acc = MetricAccumulator(type="seg", criterion=DiceCELoss(), num_classes=2)
    acc.update(logits, label)                                    # first call: library load, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            logits.sum().item()                                  # the mode does catch a host read
        acc.update(logits, label)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    s = acc.compute()
    assert math.isfinite(s["hd95_mean"]) and math.isfinite(s["asd_mean"])


def test_clipseg_test_pass_reports_the_restated_hd95_and_asd(tmp_path, monkeypatch):
    """The CLIPSeg entry point in process (the tiny synthetic configuration of tests/test_round6_gpu.py): test()'s statistics equal the restatement on what
    its accumulator received, and results.csv carries them."""
    from src.models import supervised
    from src.models.clipseg import segmentation as S
    from src.utils.tools import MetricAccumulator
    monkeypatch.chdir(tmp_path)
    made = []

    class Spy(MetricAccumulator):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

        def reset(self):                                         # one list of (preds, labels) per pass: compute() is followed by reset()
            super().reset()
            self.passes = getattr(self, "passes", [])
            self.passes.append([])

        def update(self, preds, labels):
            self.passes[-1].append((preds.detach().float().cpu().clone(), labels.detach().float().cpu().clone()))
            super().update(preds, labels)
    monkeypatch.setattr(supervised, "MetricAccumulator", Spy)
    out = S.main(["--dataset", "BUSI", "--synthetic", "--synthetic_train", "16", "--synthetic_val", "8", "--synthetic_test", "8", "--img_size", "64",
                  "--batch_size", "8", "--dtype", "fp32", "--exp", "t", "--num_workers", "0", "--epochs", "2", "--lr", "1e-3"])
    seen = made[-1].passes[-2]                                   # test()'s accumulator is created last; its pass is the one before the final reset()
    assert seen, "test() fed its accumulator nothing"
    logits = torch.cat([p for p, _ in seen])
    label = torch.cat([y for _, y in seen])
    hd, asd = R.surface_distances(logits, label, 95.0)
    st = out["test"]
    for key, vals in (("hd95", hd), ("asd", asd)):
        m, sd = R.finite_stats(vals)
        for got, want in ((st[f"{key}_mean"], m), (st[f"{key}_std"], sd)):
            assert (math.isnan(got) and math.isnan(want)) or got == pytest.approx(want, rel=1e-6, abs=1e-9), (key, got, want)
    rows = {r.split(",")[0]: r.split(",")[1:] for r in open(st["results_csv"]).read().splitlines()[1:]}
    for key, name in (("hd95", "HD95"), ("asd", "ASD")):
        if np.isfinite(hd).any():
            assert float(rows[name][0]) == pytest.approx(round(st[f"{key}_mean"], 2), abs=0.006), rows
