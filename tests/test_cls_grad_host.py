"""CPU: the CLS-sparse gradient hand-off of uia_hip.handoff (ClsGrad / publish_cls_grad / cls_grad_of) on CPU tensors: publish, take, decode, and the
guards that decide whether the head may publish one."""
import torch

from uia_hip import handoff


def _rows(B=3, D=8):
    g = torch.Generator().manual_seed(3)
    return torch.randn(B, D, generator=g), torch.randn(B, D, generator=g).bfloat16()


def test_publish_take_and_decode():
    handoff.clear()
    rows32, rows_t = _rows()
    tok = handoff.publish_cls_grad((3, 5, 8), rows32.device, rows32, rows_t)
    assert tuple(tok.shape) == (3, 5, 8) and all(s == 0 for s in tok.stride()) and bool(torch.isnan(tok).all())     # anyone but the consumer reads NaN
    cg = handoff.cls_grad_of(tok)
    assert isinstance(cg, handoff.ClsGrad) and cg.rows32 is rows32 and cg.rows_t is rows_t and cg.tokens == 5
    assert handoff.cls_grad_of(tok) is None                                        # consumed
    dense = cg.decode()
    want = torch.zeros(3, 5, 8)
    want[:, 0] = rows32
    assert dense.dtype == torch.float32 and torch.equal(dense, want)               # zeros plus a scatter


def test_token_seen_through_a_view_is_taken():
    handoff.clear()
    rows32, _ = _rows()
    tok = handoff.publish_cls_grad((3, 5, 8), rows32.device, rows32, None)
    cg = handoff.cls_grad_of(tok.permute(1, 0, 2))
    assert cg is not None and cg.rows_t is None and torch.equal(cg.decode()[:, 0], rows32)


def test_token_of_another_numel_or_registry_is_not_taken():
    handoff.clear()
    rows32, _ = _rows()
    tok = handoff.publish_cls_grad((3, 5, 8), rows32.device, rows32, None)
    assert handoff.cls_grad_of(tok[:, :2]) is None                                  # a slice: not the gradient of the whole tensor
    tok = handoff.publish_cls_grad((3, 5, 8), rows32.device, rows32, None)
    assert handoff.grad3_of(tok) is None and handoff.cls_grad_of(tok) is not None   # the three-byte registry does not know it
    assert handoff.cls_grad_of(torch.zeros(3, 5, 8)) is None                        # a real tensor
    handoff.publish_cls_grad((3, 5, 8), rows32.device, rows32, None)
    handoff.clear()
    assert not handoff.CLSG._live


def test_guards_switch_opt_in_partner_and_partner_consent():
    class VitBlockFn(torch.autograd.Function):        # stands in for the real Function: the guard goes by the node's type name and its cls_ok attribute
        @staticmethod
        def forward(ctx, x, ok):
            ctx.cls_ok = ok
            return x * 2

        @staticmethod
        def backward(ctx, g):
            return g * 2, None

    x = torch.ones(2, 3, 4, requires_grad=True)
    try:
        handoff.set_grad_resid3(True)
        y = VitBlockFn.apply(x, True)
        assert handoff.partner_node(y) is None                                      # outside a tower's block loop
        assert handoff.partner_node(y, in_chain=False) is y.grad_fn                 # the head runs behind the loop
        assert handoff.takes_cls_grad(y.permute(1, 0, 2), in_chain=False)           # through view nodes
        assert not handoff.takes_cls_grad(y + 0, in_chain=False)                    # anything else in between: no
        assert not handoff.takes_cls_grad(VitBlockFn.apply(x, False), in_chain=False)   # the partner did not consent (mask, long sequence)
        with handoff.linear_chain():
            assert handoff.takes_cls_grad(y)
        handoff.set_cls_grad(False)
        assert not handoff.takes_cls_grad(y, in_chain=False)                        # the switch
        handoff.set_cls_grad(True)
        handoff.set_grad_resid3(False)
        assert not handoff.takes_cls_grad(y, in_chain=False)                        # the per-step opt-in
    finally:
        handoff.set_cls_grad(True)
        handoff.set_grad_resid3(False)
