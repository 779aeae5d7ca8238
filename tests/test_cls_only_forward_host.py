"""CPU: the scoping of the declaration "the caller reads token 0 of this tower's output and nothing else" (handoff.cls_only, set by the engine's contrastive step
around its encode_image / encode_text calls and by nothing else), and plan-level checks that the M = B launches of the CLS-only last layer resolve to tile
configs the library already has."""
import inspect

import pytest
import torch

from uia_hip import engine, handoff, ops
from uia_hip import functional as UF


class _Tower:
    """Stands in for the model: records what its encode_* calls see."""

    def __init__(self, fail=False):
        self.seen, self.fail = [], fail

    def encode_image(self, x):
        self.seen.append(("image", handoff.cls_declared()))
        if self.fail:
            raise RuntimeError("boom")
        return x

    def encode_text(self, x):
        self.seen.append(("text", handoff.cls_declared()))
        return x


def test_the_declaration_is_set_only_inside_the_engines_encode_calls():
    assert not handoff.cls_declared()
    m = _Tower()
    x = torch.zeros(2, 3)
    assert engine._encode_image(m, x) is x and engine._encode_text(m, x) is x
    assert m.seen == [("image", True), ("text", True)] and not handoff.cls_declared()
    m.encode_image(x)                                                  # a bare call: nothing declared
    assert m.seen[-1] == ("image", False)
    # contrastive_micro reaches the towers through those two helpers only, and nothing else in the package opens the scope
    src = inspect.getsource(engine.contrastive_micro)
    assert "model.encode_image(" not in src and "model.encode_text(" not in src and "_encode_image(model" in src and "_encode_text(model" in src
    import os
    pkg = os.path.dirname(os.path.abspath(engine.__file__))
    users = [f for f in sorted(os.listdir(pkg)) if f.endswith(".py") and f != "handoff.py" and "cls_only()" in open(os.path.join(pkg, f)).read()]      # (handoff.py defines it)
    assert users == ["engine.py"], users


def test_the_declaration_is_cleared_on_exceptions():
    m = _Tower(fail=True)
    with pytest.raises(RuntimeError, match="boom"):
        engine._encode_image(m, torch.zeros(1))
    assert m.seen == [("image", True)] and not handoff.cls_declared() and not handoff.take_cls_forward()


def test_the_head_consumes_it_so_a_nested_tower_call_does_not_inherit_it():
    with handoff.cls_only():
        assert handoff.take_cls_forward()                              # the tower's head, on its way in
        assert not handoff.take_cls_forward()                          # a forward_features / encode_* call nested inside it (another consumer)
        assert not handoff.cls_declared()
    assert not handoff.take_cls_forward()
    try:
        handoff.set_cls_forward(False)                                 # the global switch: consumed all the same, never granted
        with handoff.cls_only():
            assert not handoff.take_cls_forward() and not handoff.cls_declared()
    finally:
        handoff.set_cls_forward(True)


def test_the_last_block_flag_lives_inside_the_towers_block_loop_and_is_taken_once():
    assert not handoff.take_last_block_cls() and not handoff.take_cls_rows()
    handoff.linear_chain.last_block_cls(True)
    assert not handoff.take_last_block_cls()                           # outside a block loop: never
    with handoff.linear_chain() as chain:
        chain.last_block_cls(False)
        assert not handoff.take_last_block_cls()
        chain.last_block_cls(True)
        assert handoff.take_last_block_cls() and not handoff.take_last_block_cls()      # the last block's Function, once
        handoff.cls_rows_out(True)
        assert handoff.take_cls_rows() and not handoff.take_cls_rows()                  # the adapter behind it, once
        chain.last_block_cls(True)
        handoff.cls_rows_out(True)
    assert not handoff.take_last_block_cls() and not handoff.take_cls_rows()             # the loop's exit clears what nobody took
    with handoff.linear_chain():
        assert not handoff.take_last_block_cls() and not handoff.take_cls_rows()


def test_forward_features_of_a_dense_consumer_never_asks_for_the_rows():
    """VisionTransformer.forward_features takes the rows only on its caller's word (cls_only=True, TimmModel.forward under the declaration): the default is all tokens."""
    from src.third_party.biomedclip.model import HFTextEncoder, TimmModel, VisionTransformer
    sig = inspect.signature(VisionTransformer.forward_features)
    assert sig.parameters["cls_only"].default is False
    assert "take_cls_forward()" in inspect.getsource(TimmModel.forward) and "take_cls_forward()" in inspect.getsource(HFTextEncoder.forward)
    assert "take_cls_forward" not in inspect.getsource(VisionTransformer.forward_features)


@pytest.mark.parametrize("esz", (2, 4))
@pytest.mark.parametrize("M", (12, 128, 256))
def test_the_m_equals_b_launches_resolve_to_existing_tile_configs(M, esz):
    """proj, fc1, fc2 and project2 of a ViT-B block / BERT layer at M = B: one launch each of the whole M on the small-M configs (3, or 21 for a few fp32 tiles; 4 for
    N = 64) that the backward's M = B data gradients already run on; no ring config, no K-blocked operand, no folded LayerNorm below 2049 rows."""
    dt = torch.bfloat16 if esz == 2 else torch.float32
    assert not UF.ln_fold_enabled(dt, M)
    for N, K, facts in ((768, 768, dict(out32=True, resid=True)), (3072, 768, dict(act=True, aux_out=True, out_t=True)), (768, 3072, dict(out32=True, resid=True)),
                        (768, 64, dict(out32=True, resid=True)), (64, 768, dict(out_t=True))):
        assert not ops.kb_ok(M, N, K, dt)
        plan = ops.plan_gemm(M, N, K, esz, 256, 0, packed=True, **facts)
        assert len(plan) == 1 and (plan[0].lo, plan[0].hi) == (0, M), (N, K, plan)
        cfg = ops.auto_tile_cfg(M, N, K, esz)
        assert plan[0].base == cfg and cfg in (3, 4, 21) and cfg not in ops.RING_CFGS and not plan[0].w_kblocked, (N, K, plan)


def test_the_bf16_rows_keep_the_launchers_own_choice():
    """functional._rows_tile_cfg: only the fp32 (parity) mode, on the device, borrows the dense launch's tile config; bf16 — the benchmark's mode — passes 0."""
    w = torch.zeros(768, 768)
    assert UF._rows_tile_cfg(50432, w, w, torch.bfloat16, out32=True, resid=True) == 0
    assert UF._rows_tile_cfg(50432, w, w, torch.float32, out32=True, resid=True) == 0        # a host tensor: nothing to mirror
    # what the fp32 path asks the planner: the config of the dense launch's first rows, an existing ring config above 2048 rows and the small-M one below
    big = next(L.base for L in ops.plan_gemm(2364, 768, 768, 4, 256, 0, packed=True, out32=True, resid=True) if L.lo == 0)
    small = next(L.base for L in ops.plan_gemm(384, 768, 768, 4, 256, 0, packed=True, out32=True, resid=True) if L.lo == 0)
    assert big in ops.RING_CFGS and small == ops.auto_tile_cfg(384, 768, 768, 4)
