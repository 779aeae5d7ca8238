"""ops.mona_cls_fwd (uia_mona_cls_fwd, csrc/cls_grad.hip) bit for bit against the CLS rows ops.mona_spatial_fwd writes for the same t — the token bypasses the
spatial operator, so the two are the same formula on the same operands, the dropout mask indexed in the dense [B, 1 + h·w, 64] tensor — and then ops.mona_cls_bwd
on the compact t (t_rows) against the CLS rows of the dense spatial backward, as test_cls_grad_kernels_gpu.py holds the backward on the dense t.
ops.rows3_to_f32 (the CLS rows of a three-byte tensor as fp32) against ops.three_byte_to_float."""
import pytest
import torch

pytestmark = pytest.mark.gpu


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


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dt", (torch.bfloat16, torch.float32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("B,hw", ((1, (2, 2)), (5, (14, 14))), ids=("1x2x2", "5x14x14"))
def test_mona_cls_forward_equals_the_cls_rows_of_the_dense_spatial_forward_and_feeds_the_backward(B, hw, dt):
    from uia_hip import ops
    variant = "hybrid"
    h, w = hw
    N = 1 + h * w
    g = torch.Generator().manual_seed(23 + h + B)
    P = spatial_params(variant, g)
    t = torch.randn(B * N, 64, generator=g).to(dev()).to(dt)
    t_cls = t[::N].contiguous()
    dd_cls = torch.randn(B, 64, generator=g).to(dev()).to(dt)
    dd = torch.zeros(B * N, 64, device=dev(), dtype=dt)
    dd[::N] = dd_cls
    mask = (torch.rand(B, N, 64, generator=g) >= 0.1).to(torch.uint8).to(dev())
    for name, kw in (("p_drop = 0", dict(p_drop=0.0)), ("seed", dict(p_drop=0.1, seed=0x1234ABCD5)), ("keep_mask", dict(p_drop=0.1, keep_mask=mask))):
        dense = torch.full((B * N, 64), float("nan"), device=dev(), dtype=dt)
        ops.mona_spatial_fwd(variant, B, h, w, t, P, dense, **kw)
        got = torch.full((B + 1, 64), float("nan"), device=dev(), dtype=dt)          # one guard row behind the B rows
        ops.mona_cls_fwd(B, N, t_cls, got[:B], **kw)
        torch.cuda.synchronize()
        want = dense[::N]
        assert bool(torch.isfinite(got[:B].float()).all()) and bool(torch.isnan(got[B:].float()).all()), name
        assert torch.equal(_bits(got[:B]), _bits(want)), f"{hw} {dt} {name}: {int((got[:B] != want).sum())} of {want.numel()} elements differ"
        if kw["p_drop"] > 0 and B > 1:
            assert bool((got[:B] == 0).any()) and bool((got[:B] != 0).any()), name    # the mask drops some of the 320 elements and keeps others
        # the backward on the compact t regenerates the same mask: the CLS rows of the dense spatial backward
        dense_dt = torch.full((B * N, 64), float("nan"), device=dev(), dtype=dt)
        grads = {k: torch.zeros_like(v) for k, v in P.items()}
        ops.mona_spatial_bwd(variant, B, h, w, t, P, dd, dense_dt, grads, **kw)
        got_dt = torch.full((B, 64), float("nan"), device=dev(), dtype=dt)
        ops.mona_cls_bwd(B, N, dd_cls, t_cls, got_dt, t_rows=True, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got_dt.float()).all()) and torch.equal(_bits(got_dt), _bits(dense_dt[::N])), f"{hw} {dt} {name}: backward"


def test_mona_cls_forward_refuses_bad_arguments():
    from uia_hip import _lib
    lib = _lib.lib()
    t = torch.zeros(2, 64, device=dev(), dtype=torch.bfloat16)
    d = torch.full((2, 64), float("nan"), device=dev(), dtype=torch.bfloat16)
    for args, word in (((77, 2, 5, t.data_ptr(), 64, d.data_ptr(), 0.0, 0, None), b"bad dtype"),
                       ((_lib.BF16, 0, 5, t.data_ptr(), 64, d.data_ptr(), 0.0, 0, None), b"B=0"),
                       ((_lib.BF16, 2, 5, None, 64, d.data_ptr(), 0.0, 0, None), b"null tensor"),
                       ((_lib.BF16, 2, 5, t.data_ptr(), 32, d.data_ptr(), 0.0, 0, None), b"row stride"),
                       ((_lib.BF16, 2, 5, t.data_ptr(), 64, d.data_ptr(), 1.0, 0, None), b"p_drop")):
        assert lib.uia_mona_cls_fwd(None, *args) != 0 and word in lib.uia_last_error(), word
    torch.cuda.synchronize()
    assert bool(torch.isnan(d.float()).all())


@pytest.mark.parametrize("D", (64, 768))
def test_rows3_to_f32_equals_the_decoded_rows(D):
    from uia_hip import ops
    B, N = 5, 17
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(B * N, D, generator=g) * 3).to(dev())
    hi, lo = ops.float_to_three_byte(x)
    hi, lo = hi.contiguous(), lo.contiguous()
    want = ops.three_byte_to_float(hi, lo)[::N].contiguous()
    kb = ops.KBlocked(hi.reshape(B * N, D // 32, 32).permute(1, 0, 2).contiguous())
    for name, plane in (("row-major", hi), ("K-blocked", kb)):
        got = torch.full((B + 1, D), float("nan"), device=dev())
        ops.rows3_to_f32(plane, lo, N, got[:B])
        torch.cuda.synchronize()
        assert torch.equal(got[:B].view(torch.int32), want.view(torch.int32)) and bool(torch.isnan(got[B:]).all()), name
