"""The CLS-only forward of the last layer of both towers (handoff.cls_only, set by engine.contrastive_micro), with the switch UF.set_cls_forward off and on in
one process: a whole step through engine.begin_update / contrastive_micro.

Image tower, ViT-B/16 at depth 2, B = 12 (the shapes of test_cls_sparse_backward_gpu.py).  On: the last block's projection, fc1 and fc2 forward GEMMs and its
fc2 / fc1 data gradients are launched at M = B, no ClsGrad token is published and no [B, N, D]-sized tensor is zero-filled; off: the GEMM launches are those of
the bare encode_image / encode_text step (the parent path).  Features and every adapter gradient are set against the float64 oracle, and for the features (max-norm)
and each gradient tensor   error(on) <= (1 + m)·error(off) + 2^-20·max|ref|.   m = 0.25, the project's margin for this comparison (test_cls_sparse_backward_gpu.py),
unless two ACCEPTED dense forwards — set_ln_fold on and off, scored against the same reference — already differ by more between themselves: then m is that
measured relative difference.  m, both dense errors and the table go to profiles/cls_only_fwd_parity.json.

Text tower, hidden 128, 2 heads, 2 layers, L = 32, B = 12, captions of 1, 7, 31 and 32 tokens and one all-padding caption: the same bar against the float64 text
oracle.  Fallbacks (a hook on the last block, a LoRA last block, a masked block, --unpad-text, forward_features for a dense head, a bare encode_* call) run the dense
launches.  Two on-runs with the same dropout seed give the same feature bits."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, D = 12, 197, 768
CFG = dict(embed_dim=128, vision_cfg=dict(img_size=224, patch_size=16, embed_dim=768, depth=2, num_heads=12),
           text_cfg=dict(vocab_size=30000, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, max_position_embeddings=32))
TEXT_CFG = dict(embed_dim=64, vision_cfg=dict(img_size=32, patch_size=16, embed_dim=128, depth=1, num_heads=2),
                text_cfg=dict(vocab_size=120, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=32))
MARGIN = 0.25
PARITY = os.path.join(ROOT, "profiles", "cls_only_fwd_parity.json")


def dev():
    return torch.device("cuda:0")


def batch():
    g = torch.Generator().manual_seed(5)
    images = torch.rand(B, 3, 224, 224, generator=g)
    ids = torch.zeros(B, 32, dtype=torch.long)
    ids[:, 0], ids[:, 1:6], ids[:, 6] = 2, torch.randint(1000, 30000, (B, 5), generator=g), 3
    return images, ids


def mona_model(variant, cfg=CFG, train=False):
    from src.adapters import inject_mona_variant_to_open_clip
    from src.third_party.biomedclip.model import create_biomedclip
    model = create_biomedclip(config=cfg, seed=2)
    for p in model.parameters():
        p.requires_grad_(False)
    inject_mona_variant_to_open_clip(model, variant=variant, bottleneck_dim=64)
    tg = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "mona" in k and not k.endswith(("norm.weight", "gammax")):
                p.copy_(0.05 * torch.randn(p.shape, generator=tg))
    for k, p in model.named_parameters():
        p.requires_grad_("mona" in k)
    return model.train() if train else model.eval()


class Spy:
    """GEMM launches as (phase, M, N, K, has dact), ClsGrad tokens published and zero fills of [B, N, D]-sized tensors while it is active."""

    def __init__(self, big):
        self.gemms, self.tokens, self.fills, self.phase, self.big = [], 0, [], "fwd", big

    def __enter__(self):
        from uia_hip import functional as UF
        from uia_hip import handoff, ops
        self.saved = (ops._gemm_one, UF.publish_cls_grad, torch.zeros, torch.zeros_like, handoff.ClsGrad.decode)
        og, op, oz, ozl, od = self.saved

        def gemm(a, w, **kw):
            M = a.rows if ops.is_kb(a) else a.shape[0]
            Nw, K = (w.row if isinstance(w, ops.PackedW) else w).shape if not isinstance(w, ops.ExtW) else (w.N, w.K)
            self.gemms.append((self.phase, M, Nw, K, kw.get("dact") is not None))
            return og(a, w, **kw)

        def pub(*a, **kw):
            self.tokens += 1
            return op(*a, **kw)

        def note(t):
            if t.numel() >= self.big:
                self.fills.append(tuple(t.shape))
            return t
        ops._gemm_one, UF.publish_cls_grad = gemm, pub
        torch.zeros, torch.zeros_like = (lambda *a, **kw: note(oz(*a, **kw))), (lambda *a, **kw: note(ozl(*a, **kw)))
        handoff.ClsGrad.decode = lambda s: note(od(s))
        return self

    def __exit__(self, *exc):
        from uia_hip import functional as UF
        from uia_hip import handoff, ops
        ops._gemm_one, UF.publish_cls_grad, torch.zeros, torch.zeros_like, handoff.ClsGrad.decode = self.saved
        return False

    def of(self, phase):
        return [g[1:] for g in self.gemms if g[0] == phase]


def engine_step(model, images, ids, on, ft_const=None, big=B * N * D):
    """One micro-batch through engine.begin_update / contrastive_micro on one stream.  ft_const: the text features every run of a comparison uses (the text tower's
    few-row GEMM tails sum through float atomics: two calls differ in their last bits)."""
    from uia_hip import engine
    from uia_hip import functional as UF
    from src.losses import InfoNCELoss
    for p in model.parameters():
        p.grad = None
    got = {}
    with Spy(big) as spy:
        def features(fi, ft):
            got["fi"], got["ft"] = fi.detach().float().cpu(), ft.detach().float().cpu()
            spy.phase = "bwd"
            return fi, (ft if ft_const is None else ft_const)
        try:
            UF.set_cls_forward(on)
            engine.begin_update(model)
            loss = engine.contrastive_micro(model, InfoNCELoss(0.07), images, ids, overlap_text=False, image_split=0, features=features)
            torch.cuda.synchronize()
        finally:
            engine.end_update()
            UF.set_cls_forward(True)
            UF.clear_t_copies()
    grads = {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters() if p.requires_grad and p.grad is not None}
    return dict(fi=got["fi"], ft=got["ft"], loss=float(loss), grads=grads, fwd=spy.of("fwd"), bwd=spy.of("bwd"), tokens=spy.tokens, fills=spy.fills)


def bare_step(model, images, ids, ft_const=None):
    """The parent path: encode_image / encode_text called directly between begin_update and end_update (no declaration), loss, backward."""
    from uia_hip import engine
    from uia_hip import functional as UF
    from src.losses import InfoNCELoss
    for p in model.parameters():
        p.grad = None
    with Spy(B * N * D) as spy:
        try:
            engine.begin_update(model)
            fi = model.encode_image(images)
            ft = model.encode_text(ids)
            spy.phase = "bwd"
            loss = InfoNCELoss(0.07)(fi, ft if ft_const is None else ft_const)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            engine.end_update()
            UF.clear_t_copies()
    return dict(fi=fi.detach().float().cpu(), ft=ft.detach().float().cpu(), fwd=spy.of("fwd"), bwd=spy.of("bwd"), tokens=spy.tokens)


def last_block_rows(run):
    """Rows of the LAST block's forward projection / fc1 / fc2 launches (the last launches of those shapes before the head) and of its fc2 / fc1 data gradients."""
    fwd = run["fwd"]
    last = lambda n, k: [M for M, Nw, K, _ in fwd if (Nw, K) == (n, k)][-1]
    i = next(i for i, (M, Nw, K, dact) in enumerate(run["bwd"]) if dact)
    assert run["bwd"][i][1:3] == (4 * D, D) and run["bwd"][i + 1][1:3] == (D, 4 * D)
    return (last(D, D), last(4 * D, D), last(D, 4 * D)), (run["bwd"][i][0], run["bwd"][i + 1][0])


def errors(run, ref_f, ref_g):
    e = {"features": float((run["fi"].double() - ref_f).abs().max())}
    e.update({k: float((run["grads"][k].double() - ref_g[k]).abs().max()) for k in ref_g})
    return e


def margin_of(e_fold, e_plain, refmax):
    """0.25, or the relative difference of two accepted dense forwards (LayerNorm fold on / off) where that is larger; entries at the floor say nothing."""
    m = MARGIN
    for k in e_fold:
        a, b = e_fold[k], e_plain[k]
        if min(a, b) > 2.0 ** -20 * refmax[k]:
            m = max(m, abs(a - b) / min(a, b))
    return m


def record(key, doc_entry):
    try:
        doc = json.load(open(PARITY))
    except (OSError, ValueError):
        doc = {}
    doc[key] = doc_entry
    with open(PARITY, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)


def judge(key, on, off, plain, ref_f, ref_g, shape):
    refmax = {"features": float(ref_f.abs().max())}
    refmax.update({k: float(v.abs().max()) for k, v in ref_g.items()})
    gmax = max([refmax[k] for k in ref_g] or [0.0])
    e_on, e_off, e_plain = errors(on, ref_f, ref_g), errors(off, ref_f, ref_g), errors(plain, ref_f, ref_g)
    m = margin_of(e_off, e_plain, refmax)
    table = {k: dict(on=e_on[k], off=e_off[k], off_without_ln_fold=e_plain[k], ref_max=refmax[k]) for k in sorted(e_on)}
    record(key, dict(shape=shape, margin=m, project_margin=MARGIN, largest_gradient_entry=gmax, max_abs_error_vs_float64=table))
    for k, row in table.items():
        print(f"{k:60s} on {row['on']:.3e}  off {row['off']:.3e}  off, no fold {row['off_without_ln_fold']:.3e}  |ref| {row['ref_max']:.3e}")
    print(f"margin m = {m:.3f}")
    floor = lambda k: 2.0 ** -20 * (refmax["features"] if k == "features" else gmax)
    bad = {k: row for k, row in table.items() if not row["on"] <= (1 + m) * row["off"] + floor(k)}
    assert not bad, bad


@pytest.mark.parametrize("variant,mode", (("hybrid", "bf16"), ("freq_enhanced", "bf16"), ("hybrid", "fp32")))
def test_image_tower_on_against_off_and_the_float64_oracle(variant, mode):
    """Measured on the MI355X (profiles/cls_only_fwd_parity.json).  bf16: the two accepted dense forwards differ by 1.85 x (hybrid) and 1.03 x (freq_enhanced) in
    their own gradient errors, m is that, and every tensor is within it; features on 9.22e-3 / off 9.29e-3 (hybrid), 8.59e-3 / 9.69e-3 (freq_enhanced).
    fp32: there is no LayerNorm fold, so m = 0.25.  The M = B launches of the fp32 (parity) mode run on the tile config of the dense launch they stand in for
    (functional._rows_tile_cfg), so the row-wise stages round as the dense rows do and only the attention kernel's rounding differs: features on 2.87e-6 / off
    2.62e-6 of 1.53; the tightest tensor, blocks.0 adapter_conv.freq_filter, on 1.673e-9 / off 1.294e-9 against a bar of 1.79e-9.  With the launcher's own small-M
    configs instead the same case stood at 2.349e-9 and missed the bar: these gradients are what a cancellation leaves (2e-4 relative error in fp32 in either
    run), and over other batches of this shape the on / off ratio of a tensor's error still runs from about 0.3 to 3."""
    from oracle import losses_ref, train_ref, vit_ref
    from uia_hip import functional as UF
    UF.set_compute_dtype(dict(bf16=torch.bfloat16, fp32=torch.float32)[mode])
    try:
        images, ids = batch()
        model = mona_model(variant)
        P = {k: v.detach().clone() for k, v in model.state_dict().items()}
        model = model.to(dev())
        im, tk = images.to(dev()), ids.to(dev())
        with torch.no_grad():
            ft = model.encode_text(tk).detach().clone()
        bare = bare_step(model, im, tk, ft)
        off = engine_step(model, im, tk, False, ft)
        on = engine_step(model, im, tk, True, ft)
        UF.set_ln_fold(False)
        plain = engine_step(model, im, tk, False, ft)
    finally:
        UF.set_ln_fold(True)
        UF.set_compute_dtype(torch.bfloat16)
    # off: the parent path's launches (the text tower's included) and its feature bits
    assert off["fwd"] == bare["fwd"] and off["bwd"] == bare["bwd"] and off["tokens"] == bare["tokens"] == 2 and torch.equal(off["fi"], bare["fi"])
    assert last_block_rows(off) == ((B * N, B * N, B * N), (B, B))
    # on: the last block behind its QKV GEMM at M = B, forward and backward; nothing published, nothing of the dense size filled
    assert last_block_rows(on) == ((B, B, B), (B, B)), (on["fwd"], on["bwd"])
    assert sum(1 for M, Nw, K, _ in on["fwd"] if (M, Nw, K) == (B * N, 4 * D, D)) == 1 and sum(1 for M, Nw, K, _ in off["fwd"] if (M, Nw, K) == (B * N, 4 * D, D)) == 2
    assert on["tokens"] == 0 and on["fills"] == [], (on["tokens"], on["fills"])
    names = [k for k in P if "mona" in k]
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    mona = dict(variant=variant, hw=(14, 14))
    ref_f = vit_ref.timm_vit_forward(images.double(), P64, heads=12, mona=mona)
    ref_g = train_ref.grads_of(lambda Pq, x: losses_ref.info_nce(vit_ref.timm_vit_forward(x, Pq, heads=12, mona=mona), ft.detach().cpu().double(), 0.07),
                               P64, names, [(images.double(),)])[0]
    # the spatial operator's parameters of the LAST adapter get exactly zero from the on-run, as from the CLS-sparse backward
    last = f"visual.trunk.blocks.{CFG['vision_cfg']['depth'] - 1}.mona."
    assert all(float(on["grads"][k].abs().max()) == 0.0 for k in on["grads"] if k.startswith(last) and "adapter_conv" in k)
    judge(f"image_{variant}_{mode}", on, off, plain, ref_f, ref_g, f"ViT-B/16 depth 2, B = {B}")


def text_batch():
    g = torch.Generator().manual_seed(17)
    ids = torch.zeros(B, 32, dtype=torch.long)
    for b, n in enumerate((1, 7, 31, 32, 0, 7, 32, 1, 31, 5, 16, 17)):          # caption 4 is all padding
        ids[b, :n] = torch.randint(1, 120, (n,), generator=g)
    return torch.rand(B, 3, 32, 32, generator=g), ids


@pytest.mark.parametrize("mode", ("bf16", "fp32"))
def test_text_tower_on_against_off_and_the_float64_oracle(mode):
    from oracle import text_ref
    from uia_hip import functional as UF
    UF.set_compute_dtype(dict(bf16=torch.bfloat16, fp32=torch.float32)[mode])
    try:
        images, ids = text_batch()
        model = mona_model("baseline", TEXT_CFG)
        P64 = {k: (v.detach().clone().double() if v.is_floating_point() else v.detach().clone()) for k, v in model.state_dict().items()}
        model = model.to(dev())
        im, tk = images.to(dev()), ids.to(dev())
        runs = {}
        for name, flag in (("off", False), ("on", True)):
            r = engine_step(model, im, tk, flag, big=1 << 60)
            runs[name] = dict(fi=r["ft"], grads={}, fwd=r["fwd"])
        UF.set_ln_fold(False)
        r = engine_step(model, im, tk, False, big=1 << 60)
        runs["plain"] = dict(fi=r["ft"], grads={}, fwd=r["fwd"])
    finally:
        UF.set_ln_fold(True)
        UF.set_compute_dtype(torch.bfloat16)
    Dt, Ft, M = 128, 256, B * 32
    text_rows = lambda run, n, k: [m for m, Nw, K, _ in run["fwd"] if (Nw, K) == (n, k) and m in (B, M)]
    assert text_rows(runs["off"], Ft, Dt) == [M, M] and text_rows(runs["on"], Ft, Dt) == [M, B]          # fc1 of the two layers
    assert text_rows(runs["off"], Dt, Ft) == [M, M] and text_rows(runs["on"], Dt, Ft) == [M, B]          # fc2
    ref = text_ref.bert_text_forward(ids, P64, heads=2)
    # the all-padding caption: the oracle's softmax over no key is NaN; the kernels clamp such a caption to ONE key (uia_attn_fwd), which for the CLS row is the
    # oracle on the caption cut to its first position with that position kept
    x = text_ref.bert_hidden(ids[4:5, :1], P64, 2, "text.transformer.", pad_id=-1)[:, 0]
    ref[4] = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(x, P64["text.proj.0.weight"])), P64["text.proj.2.weight"])[0]
    assert bool(torch.isfinite(ref).all())
    judge(f"text_{mode}", runs["on"], runs["off"], runs["plain"], ref, {}, f"BERT hidden 128, 2 heads, 2 layers, L = 32, B = {B}")


def test_the_residual_cls_rows_of_all_three_forms():
    """functional._res_cls_rows: normalised fp32 rows, a raw fp32 sum with statistics, a three-byte raw sum (row-major and K-blocked hi plane)."""
    from uia_hip import functional as UF
    from uia_hip import ops
    Bq, L, Dq, eps = 5, 7, 128, 1e-12
    g = torch.Generator().manual_seed(3)
    raw = (torch.randn(Bq * L, Dq, generator=g) * 2 + 0.5).to(dev())
    w, b = (1 + 0.1 * torch.randn(Dq, generator=g)).to(dev()), (0.1 * torch.randn(Dq, generator=g)).to(dev())
    ln = lambda x: torch.nn.functional.layer_norm(x.double(), (Dq,), w.double(), b.double(), eps)
    got = UF._res_cls_rows(UF.LnResidual(raw, None, w, b), L, Bq, Dq, eps)
    assert torch.equal(got, raw[::L])
    stats = torch.empty(Bq * L, 2, device=dev())
    got = UF._res_cls_rows(UF.LnResidual(raw, stats, w, b), L, Bq, Dq, eps)
    assert float((got.double() - ln(raw[::L])).abs().max()) <= 2.0 ** -20 * float(ln(raw[::L]).abs().max())
    hi, lo = ops.float_to_three_byte(raw)
    hi, lo = hi.contiguous(), lo.contiguous()
    want = ln(ops.three_byte_to_float(hi, lo)[::L])
    kb = ops.KBlocked(hi.reshape(Bq * L, Dq // 32, 32).permute(1, 0, 2).contiguous())
    for plane in (hi, kb):
        got = UF._res_cls_rows(UF.LnResidual(None, stats, w, b, Dq, eps, hi=plane, lo=lo), L, Bq, Dq, eps)
        assert float((got.double() - want).abs().max()) <= 2.0 ** -20 * float(want.abs().max())


def _lora_model():
    from src.adapters import inject_lora_to_biomedclip
    from src.third_party.biomedclip.model import create_biomedclip
    model = create_biomedclip(config=CFG, seed=2)
    for p in model.parameters():
        p.requires_grad_(False)
    inject_lora_to_biomedclip(model, lora_r=8, lora_alpha=16, lora_dropout=0.0)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "lora" in k:
                p.copy_(0.03 * torch.randn(p.shape, generator=g))
    for k, p in model.named_parameters():
        p.requires_grad_("lora" in k)
    return model.eval().to(dev())


def test_fallbacks_hook_lora_unpad_and_bare_calls_run_the_dense_launches():
    from uia_hip import functional as UF
    UF.set_compute_dtype(torch.bfloat16)
    images, ids = (t.to(dev()) for t in batch())
    model = mona_model("hybrid").to(dev())
    dense_rows = ((B * N, B * N, B * N), (B * N, B * N))
    image = lambda run: [g for g in run["fwd"] if g[2] not in (128, 256)]          # (the text tower of this geometry contracts over 128 or 256; it may still take its rows)
    # a forward hook on the last block: begin_update does not opt in to the token hand-offs either, so the whole step is the dense one
    handle = model.visual.trunk.blocks[-1].register_forward_hook(lambda m, i, o: None)
    try:
        hooked, base = engine_step(model, images, ids, True), engine_step(model, images, ids, False)
    finally:
        handle.remove()
    assert image(hooked) == image(base) and hooked["bwd"] == base["bwd"] and last_block_rows(hooked) == dense_rows and torch.equal(hooked["fi"], base["fi"])
    # --unpad-text: the packed text path keeps its dense last layer (the image tower still takes the rows)
    UF.set_unpad_text(True)
    try:
        packed_on, packed_off = engine_step(model, images, ids, True), engine_step(model, images, ids, False)
    finally:
        UF.set_unpad_text(False)
    text = lambda run: [g for g in run["fwd"] if g[2] in (128, 256) and g[1] in (128, 256, 384)]
    # (two runs of the text tower differ in the last bits of their split-K tails: the launches are compared exactly, the features to fp32 rounding)
    assert text(packed_on) == text(packed_off) and float((packed_on["ft"] - packed_off["ft"]).abs().max()) <= 2.0 ** -16 * float(packed_off["ft"].abs().max())
    # a bare encode_image / encode_text outside the engine's declaration: the parent path, bit for bit, switch on or off
    UF.set_cls_forward(True)
    with torch.no_grad():
        a_i, a_t = model.encode_image(images), model.encode_text(ids)
        UF.set_cls_forward(False)
        try:
            b_i = model.encode_image(images)
        finally:
            UF.set_cls_forward(True)
    off = engine_step(model, images, ids, False)
    assert torch.equal(a_i, b_i) and torch.equal(a_i.float().cpu(), off["fi"]) and bool(torch.isfinite(a_t).all())
    # forward_features for a dense head (segmentation, classification taps): all tokens, even inside a declared scope — only TimmModel.forward consumes it
    with torch.no_grad(), UF.cls_only():
        tokens = model.visual.trunk.forward_features(images)
    assert tuple(tokens.shape) == (B, N, D)
    # a LoRA last block
    lora = _lora_model()
    a, b = engine_step(lora, images, ids, True), engine_step(lora, images, ids, False)
    assert image(a) == image(b) and a["bwd"] == b["bwd"] and torch.equal(a["fi"], b["fi"])


def _masked_tail(mask, declared):
    """x -> VitBlockFn -> VitBlockFn(mask) -> ClsHeadFn on a small geometry, the last block told that it is the last one."""
    from uia_hip import functional as UF
    from uia_hip import handoff
    g = torch.Generator().manual_seed(31)
    Bq, Nq, Dq, Fq, E = 4, 17, 128, 512, 64
    r = lambda *s: (torch.randn(*s, generator=g) * (s[-1] ** -0.5 if len(s) > 1 else 0.1)).to(dev())
    spec = lambda m: UF.BlockSpec(2, 1e-6, "gelu", (1 + r(Dq), r(Dq)), (r(3 * Dq, Dq), r(3 * Dq)), (r(Dq, Dq), r(Dq)), (1 + r(Dq), r(Dq)), (r(Fq, Dq), r(Fq)), (r(Dq, Fq), r(Dq)), mask=m)
    s0, s1 = spec(None), spec(mask)
    ln_w, ln_b, proj = 1 + r(Dq), r(Dq), r(E, Dq)
    x = torch.randn(Bq, Nq, Dq, generator=g).to(dev()).requires_grad_(True)
    dfeat = torch.randn(Bq, E, generator=g).to(dev())
    try:
        UF.clear_t_copies()
        UF.set_grad_resid3(True)
        with handoff.linear_chain() as chain:
            y = UF.vit_block(x, s0)
            chain.last_block_cls(declared)
            y = UF.vit_block(y, s1)
        feat = UF.ClsHeadFn.apply(y, ln_w, ln_b, 1e-6, proj)
        feat.backward(dfeat)
        torch.cuda.synchronize()
    finally:
        UF.set_grad_resid3(False)
        UF.clear_t_copies()
    return tuple(y.shape), feat.detach().clone(), x.grad.detach().clone()


@pytest.mark.parametrize("mode", ("bf16", "fp32"))
def test_fallback_masked_block_runs_dense_and_the_unmasked_one_takes_the_rows(mode):
    from uia_hip import functional as UF
    UF.set_compute_dtype(dict(bf16=torch.bfloat16, fp32=torch.float32)[mode])
    try:
        s0, f0, g0 = _masked_tail("causal", False)
        s1, f1, g1 = _masked_tail("causal", True)
        assert s0 == s1 == (4, 17, 128) and torch.equal(f0, f1) and torch.equal(g0, g1)
        s2, f2, g2 = _masked_tail(None, False)
        s3, f3, g3 = _masked_tail(None, True)
        assert s2 == (4, 17, 128) and s3 == (4, 1, 128) and bool(torch.isfinite(g3).all())
        tol = 2.0 ** -7 if mode == "bf16" else 2.0 ** -18          # the rounding of the compute dtype, as the CLS-sparse backward's twin of this test
        assert float((f2 - f3).abs().max()) <= tol * float(f2.abs().max()) and float((g2 - g3).abs().max()) <= tol * float(g2.abs().max())
    finally:
        UF.set_compute_dtype(torch.bfloat16)


def test_two_on_runs_with_the_same_dropout_seed_give_the_same_feature_bits():
    from uia_hip import functional as UF
    UF.set_compute_dtype(torch.bfloat16)
    images, ids = (t.to(dev()) for t in batch())
    model = mona_model("hybrid", train=True).to(dev())
    runs = []
    for _ in range(2):
        UF.set_dropout_seed(1234)
        runs.append(engine_step(model, images, ids, True))
    assert torch.equal(runs[0]["fi"], runs[1]["fi"]) and bool(torch.isfinite(runs[0]["fi"]).all())
    assert last_block_rows(runs[0])[0] == (B, B, B)
