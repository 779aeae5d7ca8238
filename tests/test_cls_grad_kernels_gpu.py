"""The two small kernels of the CLS-sparse backward against the dense launches they stand in for, bit for bit:
  ops.mona_cls_bwd            = the CLS rows ops.mona_spatial_bwd writes when dd is zero-padded to all tokens (same formula, same operands)
  ops.layernorm_bwd_periodic  = ops.layernorm_bwd on the residual-gradient rows zero-padded to dense (adding +0.0 changes no bit)
and ops.copy_rows against torch indexing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

VARIANTS = ("baseline", "noise_aware", "freq_enhanced", "hybrid")


def dev():
    return torch.device("cuda:0")


def spatial_params(variant, g):
    r = lambda *s: (0.2 * torch.randn(*s, generator=g)).to(dev())
    P = dict(conv1_w=r(64, 1, 3, 3), conv1_b=r(64), conv2_w=r(64, 1, 5, 5), conv2_b=r(64), conv3_w=r(64, 1, 7, 7), conv3_b=r(64), proj_w=r(64, 64, 1, 1), proj_b=r(64))
    if variant in ("freq_enhanced", "hybrid"):
        P["freq"] = 1.0 + r(64)
    if variant in ("noise_aware", "hybrid"):
        P.update(ne1_w=r(16, 64, 1, 1), ne1_b=r(16), ne3_w=r(3, 16, 1, 1), ne3_b=r(3))
    return P


@pytest.mark.parametrize("dt", (torch.bfloat16, torch.float32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("hw", ((2, 2), (14, 14)), ids=("2x2", "14x14"))
@pytest.mark.parametrize("variant", VARIANTS)
def test_mona_cls_backward_equals_the_cls_rows_of_the_dense_spatial_backward(variant, hw, dt):
    from uia_hip import ops
    B, (h, w) = 3, hw
    N = 1 + h * w
    g = torch.Generator().manual_seed(11 + h)
    P = spatial_params(variant, g)
    t = torch.randn(B * N, 64, generator=g).to(dev()).to(dt)
    dd_cls = torch.randn(B, 64, generator=g).to(dev()).to(dt)
    dd = torch.zeros(B * N, 64, device=dev(), dtype=dt)
    dd[::N] = dd_cls
    mask = (torch.rand(B, N, 64, generator=g) >= 0.1).to(torch.uint8).to(dev())
    for name, kw in (("p_drop = 0", dict(p_drop=0.0)), ("regenerated mask", dict(p_drop=0.1, seed=0x1234ABCD5)), ("explicit keep_mask", dict(p_drop=0.1, keep_mask=mask))):
        dense = torch.full((B * N, 64), float("nan"), device=dev(), dtype=dt)
        grads = {k: torch.zeros_like(v) for k, v in P.items()}
        ops.mona_spatial_bwd(variant, B, h, w, t, P, dd, dense, grads, **kw)
        got = torch.full((B, 64), float("nan"), device=dev(), dtype=dt)
        ops.mona_cls_bwd(B, N, dd_cls, t, got, **kw)
        torch.cuda.synchronize()
        want = dense[::N]
        assert bool(torch.isfinite(got).all()), name
        assert torch.equal(got.view(torch.int16 if dt == torch.bfloat16 else torch.int32), want.contiguous().view(torch.int16 if dt == torch.bfloat16 else torch.int32)), \
            f"{variant} {hw} {dt} {name}: {int((got != want).sum())} of {got.numel()} elements differ"
        if kw["p_drop"] > 0:
            assert bool((got == 0).any()) and bool((got != 0).any()), name       # the mask really drops some of the 192 elements and keeps others


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else (torch.int8 if t.dtype == torch.int8 else torch.int32))


@pytest.mark.parametrize("D", (64, 768, 1024))
def test_layernorm_backward_with_a_periodic_residual_equals_the_dense_launch(D):
    """B = 2 images of N = 5 tokens; every instantiated form: bf16 with a three-byte result and fp32 x / three-byte x (row-major and K-blocked hi plane), and fp32."""
    from uia_hip import ops
    B, N = 2, 5
    M = B * N
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(M, D, generator=g) * 2 + 0.3).to(dev())
    gamma = (1 + 0.2 * torch.randn(D, generator=g)).to(dev())
    rows = torch.randn(B, D, generator=g).to(dev())
    dense = torch.zeros(M, D, device=dev())
    dense[::N] = rows
    dy32 = torch.randn(M, D, generator=g).to(dev())
    # fp32
    want32, got32 = torch.full((M, D), float("nan"), device=dev()), torch.full((M, D), float("nan"), device=dev())
    ops.layernorm_bwd(dy32, x, gamma, 1e-6, dres=dense, dx32=want32)
    ops.layernorm_bwd_periodic(dy32, x, gamma, 1e-6, rows, N, dx32=got32)
    assert torch.equal(_bits(got32), _bits(want32)), "fp32"
    # bf16, three-byte result, fp32 x
    dy = dy32.bfloat16()

    def three(xarg):
        out = []
        for fn in (lambda t, lo: ops.layernorm_bwd(dy, xarg, gamma, 1e-6, dres=dense, dx_t=t, dx_lo=lo),
                   lambda t, lo: ops.layernorm_bwd_periodic(dy, xarg, gamma, 1e-6, rows, N, dx_t=t, dx_lo=lo)):
            t = torch.full((M, D), float("nan"), device=dev(), dtype=torch.bfloat16)
            lo = torch.full((M, D), 77, device=dev(), dtype=torch.int8)
            fn(t, lo)
            out.append((t, lo))
        (wt, wlo), (gt, glo) = out
        return torch.equal(_bits(gt), _bits(wt)) and torch.equal(glo, wlo) and bool(torch.isfinite(gt.float()).all())

    assert three(x), "bf16, fp32 x"
    hi, lo = ops.float_to_three_byte(x)
    assert three((hi.contiguous(), lo.contiguous())), "bf16, three-byte x"
    kb = ops.KBlocked(hi.reshape(M, D // 32, 32).permute(1, 0, 2).contiguous())
    assert three((kb, lo.contiguous())), "bf16, three-byte x with a K-blocked hi plane"


def test_layernorm_backward_periodic_refuses_what_it_has_no_form_for():
    from uia_hip import ops
    from uia_hip._lib import UiaError
    M, D = 10, 64
    x, gamma, rows = torch.randn(M, D, device=dev()), torch.ones(D, device=dev()), torch.zeros(2, D, device=dev())
    dy = torch.randn(M, D, device=dev()).bfloat16()
    with pytest.raises(UiaError, match="three-byte result"):
        ops.layernorm_bwd_periodic(dy, x, gamma, 1e-6, rows, 5, dx32=torch.empty(M, D, device=dev()), dx_t=torch.empty(M, D, device=dev(), dtype=torch.bfloat16))
    with pytest.raises(UiaError, match="dres_rows"):
        ops.layernorm_bwd_periodic(dy.float(), x, gamma, 1e-6, rows[:1], 5, dx32=torch.empty(M, D, device=dev()))


@pytest.mark.parametrize("dt,W", ((torch.float32, 768), (torch.bfloat16, 64), (torch.bfloat16, 3072), (torch.int8, 16)))
def test_copy_rows_equals_indexing(dt, W):
    from uia_hip import ops
    N, B = 197, 5
    src = torch.randint(-100, 100, (B * N, W), device=dev()).to(dt)
    dst = ops.copy_rows(src, N, torch.empty(B, W, device=dev(), dtype=dt))
    assert torch.equal(dst, src[::N])
