"""-m gpu: uia_seg_viz against the numpy restatement (tests/seg_viz_reference.py) with exact equality of its three outputs, on both kernels and at both
ends of every buffer; the refusals of the C entry; and the smallest real loop end to end — the UNet baseline's test pass writes the reference's three
pictures per test image, the pictures carry the very masks the reported Dice / IoU were computed on, and --no-viz changes no metric."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import seg_viz_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64                                                       # bytes on either side of each output
SENTINEL = 0xA5


def dev():
    return torch.device("cuda:0")


def planted_inputs(B, Ci, S, label_dtype, seed):
    """Logits with ties, signed zeros, infinities and NaN in channel 0, channel 1 and both; images with all 256 levels (while they fit), values below 0,
    above 1, infinities and NaN; labels of 0 / 1 (and, as floats, 0.5, -1 and NaN, all of which are 'not 0')."""
    g = torch.Generator().manual_seed(seed)
    n = B * S * S
    logits = torch.randn(B, 2, S, S, generator=g)
    inf, nan = float("inf"), float("nan")
    plant = [(1.5, 1.5), (0.0, -0.0), (-0.0, 0.0), (inf, inf), (-inf, -inf), (inf, 1.0), (1.0, inf), (-inf, inf), (inf, -inf), (nan, 1.0), (1.0, nan), (nan, nan),
             (nan, inf), (inf, nan), (nan, -inf), (-inf, nan)]
    flat = logits.view(B, 2, S * S)
    for b in range(B):
        where = torch.randperm(S * S, generator=g)
        for j, (l0, l1) in enumerate(plant):
            flat[b, 0, where[j % (S * S)]], flat[b, 1, where[j % (S * S)]] = l0, l1
    images = torch.rand(B, Ci, S, S, generator=g)
    special = torch.cat([torch.tensor([1.0, 0.999999, -0.25, -1e-9, 1.0000001, 1.5, 300.0, -inf, inf, nan, -0.0]), torch.arange(256, dtype=torch.float32) / 255])
    v = images[:, 0].reshape(-1).clone()
    where = torch.randperm(n, generator=g)[:special.numel()]
    v[where] = special[:where.numel()]
    images[:, 0] = v.view(B, S, S)
    labels = (torch.rand(B, 1, S, S, generator=g) < 0.4).to(label_dtype)
    if label_dtype == torch.float32:
        lf = labels.view(-1)
        lf[torch.randperm(n, generator=g)[:3]] = torch.tensor([0.5, -1.0, nan])[:min(3, n)]
    if B > 1:
        labels[1] = 0                                            # one all-empty label
    if B > 2:
        labels[2] = 1                                            # one all-full label
    return logits, images, labels


def inside(t, shift):
    """A device copy of t that starts `shift` elements into a fresh buffer (shift 0: the allocator's alignment, 256 bytes and more)."""
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=dev())
    view = buf[shift:].view(t.shape)
    view.copy_(t)
    return view


class Guarded:
    """A uint8 output `shift` bytes behind GUARD sentinel bytes, followed by GUARD more; itself filled with the sentinel."""

    def __init__(self, shape, shift):
        self.n = int(np.prod(shape))
        self.lo = GUARD + shift
        self.buf = torch.full((self.lo + self.n + GUARD,), SENTINEL, dtype=torch.uint8, device=dev())
        self.t = self.buf[self.lo:self.lo + self.n].view(shape)

    def guards_intact(self):
        b = self.buf.cpu()
        return bool((b[:self.lo] == SENTINEL).all()) and bool((b[self.lo + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def run_case(logits, images, labels, shift, want_form):
    from uia_hip import ops
    B, _, S, _ = logits.shape
    lg, im, lb = inside(logits, shift), inside(images, shift), inside(labels, shift)
    outs = [Guarded((B, S, S, 3), shift), Guarded((B, S, S, 3), shift), Guarded((B, S, S), shift)]
    assert ops.seg_viz_form(lg, im, lb, *(o.t for o in outs)) == want_form
    ops.seg_viz(lg, im, lb, *(o.t for o in outs))
    won = (lg.argmax(dim=1) == 1).cpu().numpy()                  # the device's own argmax is the authority
    want = R.seg_viz(logits.numpy(), images.numpy(), labels.numpy(), pred_class1=won)
    for o, w, name in zip(outs, want, ("mask_rgb", "overlay_rgb", "pred")):
        got = o.t.cpu().numpy()
        assert np.array_equal(got, w), (name, tuple(logits.shape), images.shape[1], labels.dtype, shift, int((got != w).sum()))
        assert o.guards_intact(), (name, "a write outside the output")
    assert np.array_equal(won, R.class1(logits.numpy()))         # ... and the restated rule is that argmax
    return want


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("Ci", [1, 3])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [4, 5, 8, 37, 64])
def test_kernel_equals_the_restatement_on_both_paths(S, B, Ci, label_dtype):
    logits, images, labels = planted_inputs(B, Ci, S, label_dtype, seed=S * 100 + B * 10 + Ci)
    aligned = S % 4 == 0
    a = run_case(logits, images, labels, 0, 1 if aligned else 0)
    if aligned:                                                  # every input and output one element into its buffer: the other kernel, the same bytes
        b = run_case(logits, images, labels, 1, 0)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_kernel_reproduces_what_the_reference_wrote():
    from uia_hip import ops
    z = np.load(os.path.join(ROOT, "tests", "golden", "seg_viz_cases.npz"))
    n = len({k.split("_")[0] for k in z.files})
    assert n == 4
    for c in range(n):
        logits, images, labels = (torch.from_numpy(z[f"c{c}_{k}"]) for k in ("logits", "images", "labels"))
        for shift in (0, 1):
            lg, im, lb = inside(logits, shift), inside(images, shift), inside(labels, shift)
            mask, overlay, pred = ops.seg_viz(lg, im, lb)
            assert np.array_equal(mask.cpu().numpy(), z[f"c{c}_mask"]) and np.array_equal(overlay.cpu().numpy(), z[f"c{c}_overlay"])
            assert np.array_equal(pred.cpu().numpy(), z[f"c{c}_pred"])


def test_more_than_one_block_and_a_ragged_last_block():
    """S = 100: 2 500 quads per image (ten 256-thread blocks, the last one partly idle) on the aligned kernel; S = 99 on the other."""
    for S, form in ((100, 1), (99, 0)):
        logits, images, labels = planted_inputs(2, 1, S, torch.uint8, seed=S)
        run_case(logits, images, labels, 0, form)


def test_refused_arguments_launch_nothing():
    from uia_hip import _lib
    lib = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    B, S = 2, 8
    lg = torch.zeros(B, 2, S, S, device=dev())
    im = torch.zeros(B, 3, S, S, device=dev())
    lb = torch.zeros(B, 1, S, S, dtype=torch.uint8, device=dev())
    one = Guarded((B * S * S * 7 + 64,), 0)                      # all three outputs inside one sentinel-filled buffer
    m, o, p = one.t.data_ptr(), one.t.data_ptr() + B * S * S * 3, one.t.data_ptr() + B * S * S * 6
    ok = dict(B=B, C=2, Ci=3, S=S, lg=lg.data_ptr(), im=im.data_ptr(), lb=lb.data_ptr(), code=0, m=m, o=o, p=p)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.uia_seg_viz(s, v["B"], v["C"], v["Ci"], v["S"], v["lg"], v["im"], v["lb"], v["code"], v["m"], v["o"], v["p"])

    for kw in (dict(lg=None), dict(im=None), dict(lb=None), dict(m=None), dict(o=None), dict(p=None), dict(B=0), dict(B=-3), dict(S=0), dict(S=-8), dict(C=1),
               dict(C=3), dict(Ci=2), dict(Ci=4), dict(code=2), dict(code=-1), dict(o=m), dict(o=m + 1), dict(p=o + B * S * S * 3 - 1), dict(p=m),
               dict(m=lg.data_ptr()), dict(o=im.data_ptr() + 4), dict(p=lb.data_ptr() + B * S * S - 1)):
        assert call(**kw) != 0, kw
        assert lib.uia_last_error(), kw
    torch.cuda.synchronize()
    assert one.untouched()
    assert not lg.any() and not im.any() and not lb.any()
    assert call() == 0                                           # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert one.guards_intact() and not one.untouched()


def test_visualize_seg_writes_the_three_files_of_a_batch(tmp_path):
    """src.utils.tools.visualize_seg, the reference's signature: a batch in hand, logits or an arg-max mask."""
    from src.utils.tools import visualize_seg
    logits, images, labels = planted_inputs(3, 3, 37, torch.float32, seed=5)
    want = R.seg_viz(logits.numpy(), images.numpy(), labels.numpy())
    names = ["a/first.png", "second.jpg", "third"]
    visualize_seg(images.to(dev()), labels.to(dev()), logits.to(dev()), names, str(tmp_path / "one"))
    visualize_seg(images.to(dev()), labels.to(dev()), (logits.to(dev()).argmax(dim=1, keepdim=True)), names, str(tmp_path / "two"))
    for folder in ("one", "two"):
        assert sorted(os.listdir(tmp_path / folder)) == sorted(f"{s}{t}.png" for s in ("first", "second", "third") for t in ("", "_overlay", "_pred"))
        for i, stem in enumerate(("first", "second", "third")):
            for t, w in zip(("", "_overlay", "_pred"), want):
                assert np.array_equal(R.decode_png((tmp_path / folder / f"{stem}{t}.png").read_bytes()), w[i]), (folder, stem, t)


def test_a_writer_exception_surfaces_in_close(tmp_path):
    from src.utils.viz import SegVisualizer
    logits, images, labels = planted_inputs(2, 1, 8, torch.uint8, seed=1)
    viz = SegVisualizer(str(tmp_path / "absent"), max_batch=2, size=8)          # the folder does not exist: the writer fails
    viz.submit(images.to(dev()), labels.to(dev()), logits.to(dev()), ["a.png", "b.png"])
    with pytest.raises(OSError):
        viz.close()


# ------------------------------------------------------------------------------------------------ end to end on the smallest real loop
UNET = ["--synthetic", "--img_size", "64", "--synthetic_train", "8", "--synthetic_val", "4", "--synthetic_test", "5", "--batch_size", "4", "--epochs", "1",
        "--num_workers", "0"]


def _backup(exp):
    root = f"runs/{exp}/LN-INT/test"
    folders = sorted(d for d in os.listdir(root) if "_iou=" in d)
    return [os.path.join(root, d) for d in folders]


def test_unet_test_pass_writes_the_pictures_its_metrics_were_computed_on(tmp_path, monkeypatch):
    from src.datasets.segmentation import synthetic_sample
    from src.models.baselines import segmentation as cli
    monkeypatch.chdir(tmp_path)
    out = cli.main(UNET + ["--exp", "u"])
    (folder,) = _backup("u")
    stems = [f"test_{i:05d}" for i in range(5)]                  # a full batch of four and a ragged one
    files = sorted(os.listdir(os.path.join(folder, "viz")))
    assert files == sorted(f"{s}{t}.png" for s in stems for t in ("", "_overlay", "_pred")) and len(files) == 15
    assert not os.path.exists("runs/u/LN-INT/test/viz")          # moved, not copied
    dice, iou = [], []
    for i, stem in enumerate(stems):
        mask, overlay, pred = (R.decode_png(open(os.path.join(folder, "viz", f"{stem}{t}.png"), "rb").read()) for t in ("", "_overlay", "_pred"))
        image, label = synthetic_sample(64, (1 + 2) * 1000003 + i)                # the test split's seed is --seed + 2
        assert mask.shape == (64, 64, 3) and overlay.shape == (64, 64, 3) and pred.shape == (64, 64)
        assert np.array_equal(overlay[..., 2], np.floor(np.float32(255) * image[0].numpy()).astype(np.uint8))
        assert np.array_equal(mask[..., 0], 255 * label[0].numpy()) and np.array_equal(mask[..., 1], pred) and not mask[..., 2].any()
        assert set(np.unique(pred)) <= {0, 255}
        assert np.array_equal(overlay[..., 0], np.maximum(overlay[..., 2], mask[..., 0])) and np.array_equal(overlay[..., 1], np.maximum(overlay[..., 2], pred))
        p, g = pred > 0, mask[..., 0] > 0
        assert g.any()                                           # the synthetic ellipse is never empty: no image drops out of the mean
        inter, tot = float((p & g).sum()), float(p.sum()) + float(g.sum())
        dice.append(2.0 * inter / tot)
        iou.append(inter / (tot - inter))
    print(f"dice from the files {np.mean(dice)!r} / reported {out['test']['dice_mean']!r}; iou {np.mean(iou)!r} / {out['test']['iou_mean']!r}")
    assert abs(float(np.mean(np.float64(dice))) - out["test"]["dice_mean"]) <= 1e-12
    assert abs(float(np.mean(np.float64(iou))) - out["test"]["iou_mean"]) <= 1e-12
    # --test --no-viz: an empty folder, the same results.csv
    again = cli.main(UNET + ["--exp", "u", "--test", "--no-viz"])
    first, second = _backup("u")
    assert second != folder and os.listdir(os.path.join(second, "viz")) == []
    assert open(again["test"]["results_csv"], "rb").read() == open(out["test"]["results_csv"], "rb").read()
    assert os.path.dirname(again["test"]["results_csv"]) == second
