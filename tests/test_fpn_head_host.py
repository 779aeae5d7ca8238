"""src/third_party/fpn.py on the host: the feature-pyramid head that TimmCLIPAdapter and CLIPAdapter share, with the six autograd Functions it calls replaced
by plain-torch stand-ins of the same signature and a stub tower of float64 nn.Linear blocks.  Both classes and both tasks against the adapter's OWN nn modules
applied the textbook way; the walk over the three tower layouts; state-dict order and freeze sets against lists written out here; small_out_linear.

Bar 1e-9 relative in float64: only the order of sums differs (the 1x1 convolution before instead of after the interpolation, the zero-padded columns), a few
hundred terms of eps 1.1e-16 each.  The launches themselves are covered by the GPU suite."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from uia_hip import functional as UF
from src.third_party import fpn
from src.third_party.openai_clip.clip_adapter import CLIPAdapter
from src.third_party.timm.clip_adapter import TimmCLIPAdapter

B, GRID, D, REDUCE, CLASSES, IMG, PATCH = 2, 4, 32, 64, 2, 16, 4
N = 1 + GRID * GRID
DEPTH, LAYERS = 4, [0, 2]                                 # the last tap is not the last block: final tokens and taps differ
BAR = 1e-9


# ------------------------------------------------------------------------------------------------ stand-ins
class _Cast:
    @staticmethod
    def apply(x):
        return x


class _Linear:
    calls, outs = [], []                                  # (weight, bias, act, resid32 given, out32) and the result of every call, in order

    @staticmethod
    def apply(x, weight, bias, act, resid32, out32):
        _Linear.calls.append((weight, bias, act, resid32 is not None, out32))
        y = F.linear(x, weight, bias)
        y = {None: lambda t: t, "gelu": F.gelu, "relu": F.relu}[act](y)
        _Linear.outs.append(y if resid32 is None else y + resid32)
        return _Linear.outs[-1]


class _LayerNorm:
    @staticmethod
    def apply(x, w, b, eps):
        return F.layer_norm(x, (x.shape[-1],), w, b, eps)


class _Upsample:
    @staticmethod
    def apply(tok, b, h, w, H, W):
        return F.interpolate(tok.view(b, h, w, -1).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)


class _SegmentMean:
    @staticmethod
    def apply(x, b, n):
        return x.view(b, n, -1).mean(1)


class _Dropout:
    calls = []

    @staticmethod
    def apply(x, p, seed):
        _Dropout.calls.append((p, seed))
        return x


@pytest.fixture(autouse=True)
def stand_ins(monkeypatch):
    for name, fn in (("CastFn", _Cast), ("LinearTrainFn", _Linear), ("LayerNormAffineFn", _LayerNorm), ("UpsampleBilinearFn", _Upsample),
                     ("SegmentMeanFn", _SegmentMean), ("DropoutFn", _Dropout)):
        monkeypatch.setattr(UF, name, fn)
    _Linear.calls.clear()
    _Linear.outs.clear()
    _Dropout.calls.clear()


# ------------------------------------------------------------------------------------------------ stub towers
class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(D, D, dtype=torch.float64)
        self.seen, self.out = [], None

    def forward(self, x):
        self.seen.append(tuple(x.shape))
        self.out = x + torch.tanh(self.fc(x))
        return self.out


class _Tower(nn.Module):
    """layout "trunk": visual.trunk.{embed_tokens, blocks, embed_dim}; "batch_first" / "sequence_first": visual.{embed, batch_first, transformer.{resblocks, width}}."""

    def __init__(self, layout):
        super().__init__()
        self.proj = nn.Linear(3 * PATCH * PATCH, D, dtype=torch.float64)
        self.cls = nn.Parameter(torch.randn(D, dtype=torch.float64))
        body = nn.Module()
        setattr(body, "blocks" if layout == "trunk" else "resblocks", nn.Sequential(*[_Block() for _ in range(DEPTH)]))
        body.embed_dim = body.width = D
        if layout == "trunk":
            body.embed_tokens = self.tokens
            self.trunk = body
            self.transformer = None                       # 'trunk' comes first: this is never looked at
        else:
            self.embed = self.tokens
            self.transformer = body
            self.batch_first = layout == "batch_first"

    def tokens(self, x):
        b = x.shape[0]
        p = x.view(b, 3, GRID, PATCH, GRID, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(b, GRID * GRID, -1)
        return torch.cat([self.cls.expand(b, 1, D), self.proj(p)], 1)

    def blocks(self):
        return self.trunk.blocks if hasattr(self, "trunk") else self.transformer.resblocks


def _images(seed=1):
    return torch.rand(B, 3, IMG, IMG, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _walk(tower, images):
    """The blocks' outputs by a plain loop (the stub blocks act on the last dimension: any layout gives the same numbers), batch-first."""
    x, outs = tower.tokens(images), []
    for blk in tower.blocks():
        x = x + torch.tanh(blk.fc(x))
        outs.append(x)
    return outs


def _clip(layout):
    torch.manual_seed(0)
    clip = nn.Module()
    clip.visual = _Tower(layout)
    return clip


def _adapter(cls, task, layout):
    clip = _clip(layout)
    torch.manual_seed(1)
    return cls(clip, extract_layers=LAYERS, reduce_dim=REDUCE, num_classes=CLASSES, img_size=IMG, patch_size=PATCH, task=task).double().eval()


def rel(a, b):
    return float((a - b).detach().abs().max() / b.detach().abs().max())


# ------------------------------------------------------------------------------------------------ the walk
@pytest.mark.parametrize("layout", ["trunk", "batch_first", "sequence_first"])
def test_tapped_tokens_gives_batch_first_views_of_the_listed_blocks_outputs(layout):
    tower, images = _clip(layout).visual, _images()
    with torch.no_grad():
        final, taps = fpn.tapped_tokens(tower, images, LAYERS)
        want = _walk(tower, images)
    blocks = tower.blocks()
    fed = (N, B, D) if layout == "sequence_first" else (B, N, D)
    assert all(blk.seen == [fed] for blk in blocks)                                   # every block once, on its own layout
    assert len(taps) == len(LAYERS) and tuple(final.shape) == (B, N, D)
    for tap, i in zip(taps, LAYERS):
        assert tuple(tap.shape) == (B, N, D) and torch.equal(tap, want[i])
        assert tap.data_ptr() == blocks[i].out.data_ptr()                             # a view of what the block returned, not a copy
    assert torch.equal(final, want[-1]) and final.data_ptr() == blocks[-1].out.data_ptr()


def test_tapped_tokens_refuses_an_unknown_layout():
    with pytest.raises(AttributeError, match="neither 'trunk' nor 'transformer'"):
        fpn.tapped_tokens(nn.Module(), _images(), LAYERS)


def test_extract_vit_features_keeps_each_class_its_documented_layout():
    images = _images()
    for cls, layout, shape in ((TimmCLIPAdapter, "trunk", (B, N, D)), (TimmCLIPAdapter, "batch_first", (B, N, D)), (TimmCLIPAdapter, "sequence_first", (B, N, D)),
                               (CLIPAdapter, "sequence_first", (N, B, D))):
        ad = _adapter(cls, "seg", layout)
        with torch.no_grad():
            final, taps = ad.extract_vit_features(images)
            want = _walk(ad.clip_model.visual, images)
        assert tuple(final.shape) == shape and [tuple(t.shape) for t in taps] == [shape] * len(LAYERS), (cls.__name__, layout)
        back = (lambda t: t.permute(1, 0, 2)) if shape == (N, B, D) else (lambda t: t)
        assert torch.equal(back(final), want[-1]) and all(torch.equal(back(t), want[i]) for t, i in zip(taps, LAYERS))


# ------------------------------------------------------------------------------------------------ the head against its own nn modules
def _textbook(ad, images):
    taps = _walk(ad.clip_model.visual, images)
    a = None
    for i in reversed(range(len(LAYERS))):
        y = ad.blocks[i](ad.reduces[i](taps[LAYERS[i]][:, 1:, :]))
        a = y if a is None else y + a
    grid = a.permute(0, 2, 1).reshape(B, REDUCE, GRID, GRID)
    return ad.seg_head(grid) if ad.task == "seg" else ad.cls_head(grid)


def _head_grads(ad, out, weight):
    for p in ad.parameters():
        p.grad = None
    (out * weight).sum().backward()
    return {k: None if p.grad is None else p.grad.clone() for k, p in ad.named_parameters() if not k.startswith("clip_model.")}


@pytest.mark.parametrize("task", ["seg", "cls"])
@pytest.mark.parametrize("cls,layout", [(TimmCLIPAdapter, "trunk"), (TimmCLIPAdapter, "batch_first"), (TimmCLIPAdapter, "sequence_first"), (CLIPAdapter, "sequence_first")],
                         ids=["timm-trunk", "timm-batch_first", "timm-sequence_first", "openai"])
def test_output_and_head_gradients_equal_the_adapters_own_modules(cls, layout, task):
    ad, images = _adapter(cls, task, layout), _images()
    got, want = ad(images), _textbook(ad, images)
    assert tuple(got.shape) == ((B, CLASSES, IMG, IMG) if task == "seg" else (B, CLASSES)) and got.dtype == torch.float64
    assert rel(got, want) <= BAR, rel(got, want)
    weight = torch.randn(got.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    g_got, g_want = _head_grads(ad, got, weight), _head_grads(ad, want, weight)
    used = {"reduces", "blocks", "seg_head" if task == "seg" else "cls_head"}
    for k in g_want:
        if k.split(".")[0] in used:
            assert rel(g_got[k], g_want[k]) <= BAR, (k, rel(g_got[k], g_want[k]))
        else:
            assert g_got[k] is None and g_want[k] is None, k
    assert not _Dropout.calls                                                         # eval()


def _names(ad):
    """Every LinearTrainFn call so far as (parameter name, or the shape of an operand that is no parameter; act; residual given; fp32 output)."""
    by_id = {id(p): k for k, p in ad.named_parameters()}
    return [(by_id.get(id(w), tuple(w.shape)), act, resid, out32) for w, _, act, resid, out32 in _Linear.calls]


def test_the_launch_order_of_a_forward_is_the_written_one(monkeypatch):
    """Deep to shallow, the running sum as the residual from the second level on, then the head; a seed is drawn once, in training with p > 0 only."""
    seeds = []
    monkeypatch.setattr(UF, "_next_seed", lambda: seeds.append(len(seeds) + 7) or seeds[-1])
    pyramid = [("reduces.1.weight", None, False, True), ("blocks.1.1.weight", "gelu", False, False), ("blocks.1.3.weight", None, False, True),
               ("reduces.0.weight", None, False, True), ("blocks.0.1.weight", "gelu", False, False), ("blocks.0.3.weight", None, True, True)]
    padded = ((64, REDUCE), None, False, True)                                       # CLASSES rows zero-padded to 64: no parameter
    heads = {(TimmCLIPAdapter, "seg"): [padded], (TimmCLIPAdapter, "cls"): [padded],
             (CLIPAdapter, "seg"): [padded], (CLIPAdapter, "cls"): [("cls_head.2.weight", "relu", False, False), padded]}
    for (cls, task), head in heads.items():
        ad = _adapter(cls, task, "sequence_first")
        for training in (False, True):
            ad.train(training)
            _Linear.calls.clear(), _Dropout.calls.clear(), seeds.clear()
            ad(_images())
            assert _names(ad) == pyramid + head, (cls.__name__, task)
            p = 0.5 if cls is TimmCLIPAdapter else 0.1
            assert (_Dropout.calls, seeds) == (([(p, 7)], [7]) if training and task == "cls" else ([], [])), (cls.__name__, task, training)
        ad.cls_head[-2].p = 0.0                                                       # p = 0: no launch and no seed even in training
        _Dropout.calls.clear(), seeds.clear()
        ad(_images())
        assert not _Dropout.calls and not seeds
    with pytest.raises(ValueError, match="Invalid task type: det"):
        _adapter(CLIPAdapter, "det", "sequence_first")(_images())


# ------------------------------------------------------------------------------------------------ order and freeze rule
PYRAMID_KEYS = ["reduces.0.weight", "reduces.0.bias", "reduces.1.weight", "reduces.1.bias",
                "blocks.0.0.weight", "blocks.0.0.bias", "blocks.0.1.weight", "blocks.0.1.bias", "blocks.0.3.weight", "blocks.0.3.bias",
                "blocks.1.0.weight", "blocks.1.0.bias", "blocks.1.1.weight", "blocks.1.1.bias", "blocks.1.3.weight", "blocks.1.3.bias"]
SEG_KEYS = ["seg_head.1.weight", "seg_head.1.bias"]
CLS_KEYS = {TimmCLIPAdapter: ["cls_head.3.weight", "cls_head.3.bias"],
            CLIPAdapter: ["cls_head.2.weight", "cls_head.2.bias", "cls_head.5.weight", "cls_head.5.bias"]}
KEPT = {TimmCLIPAdapter: ["clip_model.x.mona.w", "clip_model.x.lora_A", "clip_model.x.adapter.w"], CLIPAdapter: ["clip_model.x.mona.w"]}


@pytest.mark.parametrize("cls", [TimmCLIPAdapter, CLIPAdapter])
def test_state_dict_order_is_backbone_pyramid_seg_head_cls_head(cls):
    ad = _adapter(cls, "seg", "sequence_first")
    keys = list(ad.state_dict())
    n_backbone = len(ad.clip_model.state_dict())
    assert all(k.startswith("clip_model.") for k in keys[:n_backbone])
    assert keys[n_backbone:] == PYRAMID_KEYS + SEG_KEYS + CLS_KEYS[cls]
    assert [k for k, _ in ad.named_parameters()] == keys                              # the order FlatAdapterOptimizer lays its flat buffers out in


@pytest.mark.parametrize("task", ["seg", "cls"])
@pytest.mark.parametrize("cls", [TimmCLIPAdapter, CLIPAdapter])
def test_freeze_clip_backbone_leaves_the_written_names_trainable(cls, task):
    clip = _clip("sequence_first")
    clip.x = nn.Module()
    clip.x.mona, clip.x.adapter = nn.Module(), nn.Module()
    clip.x.mona.w, clip.x.adapter.w, clip.x.lora_A, clip.x.plain = (nn.Parameter(torch.zeros(2)) for _ in range(4))
    ad = cls(clip, extract_layers=LAYERS, reduce_dim=REDUCE, num_classes=CLASSES, img_size=IMG, task=task)
    assert {"clip_model.x.mona.w", "clip_model.x.lora_A", "clip_model.x.adapter.w", "clip_model.x.plain"} <= {k for k, _ in ad.named_parameters()}
    for p in ad.parameters():
        p.requires_grad = False
    ad.freeze_clip_backbone()
    got = {k for k, p in ad.named_parameters() if p.requires_grad}
    assert got == set(KEPT[cls] + PYRAMID_KEYS + (SEG_KEYS if task == "seg" else CLS_KEYS[cls]))
    ad.task = "det"
    with pytest.raises(ValueError, match="Invalid task type: det"):
        ad.freeze_clip_backbone()


# ------------------------------------------------------------------------------------------------ small_out_linear
def test_small_out_linear_pads_two_rows_and_hands_the_gradient_to_the_unpadded_weight():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 8, generator=g, dtype=torch.float64)
    w = nn.Parameter(torch.randn(2, 8, generator=g, dtype=torch.float64))
    b = nn.Parameter(torch.randn(2, generator=g, dtype=torch.float64))
    y = fpn.small_out_linear(x, w, b)
    assert tuple(y.shape) == (5, 2) and y.is_contiguous() and torch.equal(y, (x @ w.T + b).detach())
    (wp, bp, act, resid, out32), = _Linear.calls
    assert tuple(wp.shape) == (64, 8) and tuple(bp.shape) == (64,) and (act, resid, out32) == (None, False, True)
    assert torch.equal(wp[:2], w) and not wp[2:].any() and torch.equal(bp[:2], b) and not bp[2:].any()
    dy = torch.randn(5, 2, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    assert tuple(w.grad.shape) == (2, 8) and rel(w.grad, dy.T @ x) <= BAR and rel(b.grad, dy.sum(0)) <= BAR
    _Linear.calls.clear()
    assert tuple(fpn.small_out_linear(x, w, None).shape) == (5, 2) and _Linear.calls[0][1] is None


def test_small_out_linear_hands_a_multiple_of_64_rows_over_as_the_parameter_itself():
    x = torch.randn(5, 8, dtype=torch.float64)
    w, b = nn.Parameter(torch.randn(64, 8, dtype=torch.float64)), nn.Parameter(torch.randn(64, dtype=torch.float64))
    y = fpn.small_out_linear(x, w, b)
    (wp, bp, act, resid, out32), = _Linear.calls
    assert wp is w and bp is b and (act, resid, out32) == (None, False, True)
    assert y is _Linear.outs[0]                                                       # nothing sliced off the result
