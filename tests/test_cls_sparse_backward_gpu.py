"""The whole backward with and without the CLS-sparse hand-off (handoff.ClsGrad), in one process: ViT-B/16 geometry at depth 2, B = 12 (2364 rows).

The forward is untouched, so image features must be bit-identical (and the loss, up to the order of the loss kernel's own atomic sum: same_forward).  The sparse run must launch the last block's fc2 / fc1 data gradients at M = B, the dense
run at M = B·N.  Gradients: both runs are set against a float64 restatement of the same step (oracle/vit_ref + losses_ref on the CPU, the text features the GPU
produced as a constant); for every adapter tensor the sparse path's max-norm error may exceed the dense path's by at most 25 % plus 2^-20 of the step's largest gradient
entry (the bf16 products are the same, only fp32 summation order changes; a dropped or doubled term would move the error by the size of the gradient).  Both error
tables go to profiles/cls_sparse_bwd_parity.json.

Fallbacks (a hook on the last block, the per-step opt-in off, a LoRA tower, a masked block) must take the dense path: no token is published, the launches are the dense
run's.  Data gradients are compared bit for bit; adapter WEIGHT gradients add up through float atomics (uia_wgrad, the Mona row kernels: functional.set_deterministic's
note), so two dense runs of the same step already differ in their last bits — they are held to the reordering bound of an fp32 sum over the B·N rows instead
(same_weight_gradients), next to the assertion that the launches themselves are the dense run's."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, D = 12, 197, 768
CFG = dict(embed_dim=128, vision_cfg=dict(img_size=224, patch_size=16, embed_dim=768, depth=2, num_heads=12),
           text_cfg=dict(vocab_size=30000, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, max_position_embeddings=32))
_REF = {}


def dev():
    return torch.device("cuda:0")


def batch():
    g = torch.Generator().manual_seed(5)
    images = torch.rand(B, 3, 224, 224, generator=g)
    ids = torch.zeros(B, 32, dtype=torch.long)
    ids[:, 0], ids[:, 1:6], ids[:, 6] = 2, torch.randint(1000, 30000, (B, 5), generator=g), 3
    return images, ids


def mona_model(variant):
    from src.adapters import inject_mona_variant_to_open_clip
    from src.third_party.biomedclip.model import create_biomedclip
    model = create_biomedclip(config=CFG, seed=2)
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
    return model.eval()


_TEXT = {}


def text_features(model, ids):
    """The frozen text tower's features, once per model: its few-row GEMM tails sum through float atomics (functional.set_deterministic), so two calls differ in
    their last bits — every run of a comparison gets the same operand."""
    if id(model) not in _TEXT:
        _TEXT.clear()
        with torch.no_grad():
            _TEXT[id(model)] = model.encode_text(ids).detach().clone()
    return _TEXT[id(model)]


def step(model, images, ids, cls_flag, opt_in=True):
    """One forward + backward as the engine's step brackets it (begin_update decides the per-step opt-in: hook-free towers only).  Returns features, loss, gradients,
    the GEMM launches of the backward as (M, N, K, has dact) and the number of ClsGrad tokens published."""
    from uia_hip import engine, ops
    from uia_hip import functional as UF
    from src.losses import InfoNCELoss
    for p in model.parameters():
        p.grad = None
    launches, tokens = [], []
    orig_gemm, orig_pub = ops._gemm_one, UF.publish_cls_grad

    def spy(a, w, **kw):
        M = a.rows if ops.is_kb(a) else a.shape[0]
        Nw, K = (w.row if isinstance(w, ops.PackedW) else w).shape if not isinstance(w, ops.ExtW) else (w.N, w.K)
        launches.append((M, Nw, K, kw.get("dact") is not None))
        return orig_gemm(a, w, **kw)

    def pub(*a, **kw):
        tokens.append(a[0])
        return orig_pub(*a, **kw)
    old = engine.GRAD_RESID3
    try:
        UF.set_cls_grad(cls_flag)
        engine.GRAD_RESID3 = opt_in
        engine.begin_update(model)
        ft = text_features(model, ids)
        fi = model.encode_image(images)
        loss = InfoNCELoss(0.07)(fi, ft)
        ops._gemm_one, UF.publish_cls_grad = spy, pub
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops._gemm_one, UF.publish_cls_grad = orig_gemm, orig_pub
        engine.GRAD_RESID3 = old
        engine.end_update()
        UF.set_cls_grad(True)
        UF.clear_t_copies()
    grads = {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters() if p.requires_grad}
    return dict(fi=fi.detach().float().cpu(), ft=ft.detach().float().cpu(), loss=loss.detach().float().cpu(), grads=grads, gemms=launches, tokens=len(tokens))


def same_forward(a, b):
    """Image features bit for bit.  The loss is a function of the (identical) features alone, but uia_infonce adds its 2·B row terms into one float with atomics, in
    whatever order they arrive: two evaluations of the SAME operands may differ by the rounding of that sum, at most one ulp per term."""
    la, lb = float(a["loss"]), float(b["loss"])
    return torch.equal(a["fi"], b["fi"]) and abs(la - lb) <= 2 * B * 2.0 ** -24 * abs(la)


def float64_gradients(variant, mode, P, images, ft):
    """The same step in float64 on the CPU (computed once per case): oracle ViT + Mona forward, InfoNCE against the text features the GPU produced, autograd."""
    if (variant, mode) not in _REF:
        from oracle import losses_ref, train_ref, vit_ref
        names = [k for k in P if "mona" in k]
        P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
        mona = dict(variant=variant, hw=(14, 14))
        _REF[variant, mode] = train_ref.grads_of(lambda Pq, im: losses_ref.info_nce(vit_ref.timm_vit_forward(im, Pq, heads=12, mona=mona), ft.double(), 0.07),
                                           P64, names, [(images.double(),)])[0]
    return _REF[variant, mode]


def mlp_dgrad_rows(gemms):
    """M of the LAST block's fc2 data gradient (the first launch of the backward with GELU') and of the fc1 data gradient right behind it."""
    i = next(i for i, (M, Nw, K, dact) in enumerate(gemms) if dact)
    assert gemms[i][1:3] == (4 * D, D) and gemms[i + 1][1:3] == (D, 4 * D), gemms[i:i + 2]
    return gemms[i][0], gemms[i + 1][0]


@pytest.mark.parametrize("variant,mode", (("hybrid", "bf16"), ("freq_enhanced", "bf16"), ("hybrid", "fp32")))
def test_sparse_backward_equals_the_dense_one_to_the_dense_paths_own_error(variant, mode):
    from uia_hip import functional as UF
    dt = dict(bf16=torch.bfloat16, fp32=torch.float32)[mode]
    UF.set_compute_dtype(dt)
    try:
        images, ids = batch()
        model = mona_model(variant)
        P = {k: v.detach().clone() for k, v in model.state_dict().items()}
        model = model.to(dev())
        dense = step(model, images.to(dev()), ids.to(dev()), False)
        sparse = step(model, images.to(dev()), ids.to(dev()), True)
    finally:
        UF.set_compute_dtype(torch.bfloat16)
    assert same_forward(dense, sparse)                                                                  # the forward is untouched
    assert dense["tokens"] == 0 and mlp_dgrad_rows(dense["gemms"]) == (B * N, B * N)
    assert sparse["tokens"] == 2 and mlp_dgrad_rows(sparse["gemms"]) == (B, B)                          # head -> adapter 1 -> block 1
    ref = float64_gradients(variant, mode, P, images, dense["ft"])
    gmax = max(float(v.abs().max()) for v in ref.values())
    floor = 2.0 ** -20 * gmax
    table = {}
    for k in sorted(ref):
        table[k] = dict(dense=float((dense["grads"][k].double() - ref[k]).abs().max()), sparse=float((sparse["grads"][k].double() - ref[k]).abs().max()),
                        ref_max=float(ref[k].abs().max()))
    path = os.path.join(ROOT, "profiles", "cls_sparse_bwd_parity.json")
    try:
        doc = json.load(open(path))
    except (OSError, ValueError):
        doc = {}
    doc[f"{variant}_{mode}"] = dict(shape=f"ViT-B/16 depth 2, B = {B}", largest_gradient_entry=gmax, floor=floor, margin=0.25, max_abs_error_vs_float64=table)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    for k, row in table.items():
        print(f"{k:60s} dense {row['dense']:.3e}  sparse {row['sparse']:.3e}  |ref| {row['ref_max']:.3e}")
    bad = {k: row for k, row in table.items() if not row["sparse"] <= 1.25 * row["dense"] + floor}
    assert not bad, bad


def same_weight_gradients(a, b):
    """Two runs of the SAME launches: the weight gradients are sums over the B·N rows that uia_wgrad and the Mona row kernels add up through float atomics, in
    whatever order the workgroups arrive.  Reordering a sum of n fp32 terms moves it by at most n·2^-24 of the terms' magnitude, taken here as the largest entry."""
    gmax = max(float(v.abs().max()) for v in a.values())
    return all(float((a[k] - b[k]).abs().max()) <= B * N * 2.0 ** -24 * gmax for k in a)


def test_fallbacks_hook_and_opt_in_take_the_dense_path():
    from uia_hip import functional as UF
    UF.set_compute_dtype(torch.bfloat16)
    images, ids = (t.to(dev()) for t in batch())
    model = mona_model("hybrid").to(dev())
    off = step(model, images, ids, True, opt_in=False)                       # the per-step opt-in off
    handle = model.visual.trunk.blocks[-1].register_forward_hook(lambda m, i, o: None)
    try:
        hooked = step(model, images, ids, True)                              # a forward hook on the last block: the step does not opt in
        hooked_dense = step(model, images, ids, False)
    finally:
        handle.remove()
    for name, run, base in (("opt-in off", off, step(model, images, ids, False, opt_in=False)), ("hook", hooked, hooked_dense)):
        assert run["tokens"] == 0 and run["gemms"] == base["gemms"], name
        assert mlp_dgrad_rows(run["gemms"]) == (B * N, B * N), name
        assert same_forward(run, base), name
        assert same_weight_gradients(run["grads"], base["grads"]), name


def test_fallback_lora_tower_takes_the_dense_path():
    from uia_hip import functional as UF
    from src.adapters import inject_lora_to_biomedclip
    from src.third_party.biomedclip.model import create_biomedclip
    UF.set_compute_dtype(torch.bfloat16)
    images, ids = (t.to(dev()) for t in batch())
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
    model = model.eval().to(dev())
    a, b = step(model, images, ids, False), step(model, images, ids, True)
    assert b["tokens"] == 0 and a["gemms"] == b["gemms"] and sum(1 for M, _, _, _ in b["gemms"] if M == B) == 1        # the head's own data gradient, nothing else
    assert same_forward(a, b) and same_weight_gradients(a["grads"], b["grads"])


def _two_blocks(mask, cls_flag):
    """x -> VitBlockFn -> VitBlockFn(mask) -> ClsHeadFn on a small geometry (B = 4, N = 17, D = 128, two heads of 64), frozen weights: the data gradient of x."""
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
    tokens, orig = [], UF.publish_cls_grad
    UF.publish_cls_grad = lambda *a, **kw: (tokens.append(1), orig(*a, **kw))[1]
    try:
        UF.set_cls_grad(cls_flag)
        UF.clear_t_copies()
        UF.set_grad_resid3(True)
        with handoff.linear_chain():
            y = UF.vit_block(UF.vit_block(x, s0), s1)
        feat = UF.ClsHeadFn.apply(y, ln_w, ln_b, 1e-6, proj)
        feat.backward(dfeat)
        torch.cuda.synchronize()
    finally:
        UF.publish_cls_grad = orig
        UF.set_grad_resid3(False)
        UF.set_cls_grad(True)
        UF.clear_t_copies()
    return feat.detach().clone(), x.grad.detach().clone(), len(tokens)


@pytest.mark.parametrize("mode", ("bf16", "fp32"))
def test_fallback_masked_block_takes_the_dense_path_bit_for_bit(mode):
    from uia_hip import functional as UF
    UF.set_compute_dtype(dict(bf16=torch.bfloat16, fp32=torch.float32)[mode])
    try:
        f0, g0, t0 = _two_blocks("causal", False)
        f1, g1, t1 = _two_blocks("causal", True)
        assert t0 == 0 and t1 == 0 and torch.equal(f0, f1) and torch.equal(g0, g1) and bool(torch.isfinite(g1).all())
        # the same harness without the mask does take the sparse path, and agrees with the dense one to the rounding of the compute dtype
        f2, g2, t2 = _two_blocks(None, False)
        f3, g3, t3 = _two_blocks(None, True)
        assert t2 == 0 and t3 == 1 and torch.equal(f2, f3) and bool(torch.isfinite(g3).all())
        tol = 2.0 ** -7 if mode == "bf16" else 2.0 ** -18
        assert float((g2 - g3).abs().max()) <= tol * float(g2.abs().max())
    finally:
        UF.set_compute_dtype(torch.bfloat16)
