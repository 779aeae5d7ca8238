"""uia_hip.handoff on the host: the rules of the five channels that carry tensors beside autograd (token registries, T copies, the rows hand-off,
the row-sum arena) and the K-blocked save/restore, on CPU tensors of a few dozen elements.  The launches they feed are covered by the GPU suite."""
import pytest
import torch

from uia_hip import functional as UF
from uia_hip import handoff, ops
from uia_hip._lib import UiaError

CPU = torch.device("cpu")
BF16 = torch.bfloat16


@pytest.fixture(autouse=True)
def _empty_channels():
    handoff.clear()
    yield
    handoff.clear()


def _planes():
    return torch.zeros(6, 4, dtype=BF16), torch.zeros(6, 4, dtype=torch.int8)


# ------------------------------------------------------------------------------------------------ token registries
REGISTRIES = pytest.mark.parametrize("reg", [handoff.GRAD3, handoff.FWD3], ids=["grad3", "fwd3"])


def test_the_two_registries_keep_their_pool_sizes():
    assert (handoff.GRAD3.size, handoff.FWD3.size) == (64, 256) and type(handoff.GRAD3) is type(handoff.FWD3)


@REGISTRIES
def test_a_token_is_one_nan_of_the_requested_shape_found_once_behind_views(reg):
    payload = object()
    tok = reg.publish((2, 3, 4), CPU, payload)
    assert tuple(tok.shape) == (2, 3, 4) and tok.stride() == (0, 0, 0) and bool(torch.isnan(tok).all())
    assert reg.take(torch.zeros(2, 3, 4)) is None                              # an ordinary tensor of the same shape
    assert reg.take(torch.full((), float("nan")).expand(2, 3, 4)) is None      # ... and a stride-0 one that is no token
    seen = tok.permute(1, 0, 2).permute(2, 0, 1).permute(1, 2, 0)
    assert reg.take(seen) is payload
    assert reg.take(seen) is None and reg.take(tok) is None                    # consumed by the first lookup


@REGISTRIES
def test_a_token_with_a_size_one_leading_dimension_is_found_through_a_permute(reg):
    payload = object()
    one = reg.publish((1, 6, 4), CPU, payload)                                 # a one-image slice: the size-1 dimension keeps a non-zero stride
    assert reg.take(one.permute(1, 0, 2)) is payload


@REGISTRIES
def test_a_view_of_a_token_with_fewer_elements_is_not_the_token(reg):
    tok = reg.publish((2, 3, 4), CPU, object())
    assert reg.take(tok[:1]) is None                                           # same address, other numel


@REGISTRIES
def test_consecutive_tokens_differ_in_address_and_clear_forgets_them(reg):
    a, b = object(), object()
    ta, tb = reg.publish((2, 3, 4), CPU, a), reg.publish((2, 3, 4), CPU, b)
    assert ta.data_ptr() != tb.data_ptr()
    assert reg.take(tb) is b and reg.take(ta) is a
    tc = reg.publish((2, 3, 4), CPU, a)
    handoff.clear()
    assert reg.take(tc) is None


@REGISTRIES
def test_past_its_bound_the_registry_still_answers_for_the_newest_token(reg):
    toks = [reg.publish((2, 3), CPU, i) for i in range(reg.size + 1)]          # none looked up: the bound drops the old ones
    assert toks[-1].data_ptr() == toks[0].data_ptr()                           # the ring of NaNs has wrapped
    assert reg.take(toks[-1]) == reg.size
    assert reg.take(toks[1]) is None
    newest = reg.publish((2, 3), CPU, "newest")
    assert reg.take(newest) == "newest"


def test_the_public_lookups_return_named_tuples_of_the_very_planes():
    hi, lo = _planes()
    sums = torch.zeros(6, 2, dtype=torch.int64)
    got = UF.grad3_of(UF.publish_grad3((2, 3, 4), CPU, hi, lo).permute(1, 0, 2))
    assert isinstance(got, tuple) and isinstance(got, handoff.Resid3) and len(got) == 2
    g_hi, g_lo = got
    assert g_hi is hi and g_lo is lo and got[0] is hi and got.lo is lo
    got = UF.fwd3_of(UF.publish_fwd3((2, 3, 4), CPU, hi, lo, sums))
    assert isinstance(got, tuple) and len(got) == 3
    f_hi, f_lo, f_sums = got
    assert f_hi is hi and f_lo is lo and f_sums is sums
    assert isinstance(got.resid3, handoff.Resid3) and got.resid3.hi is hi and got.resid3.lo is lo
    assert UF.grad3_of(UF.publish_fwd3((2, 3, 4), CPU, hi, lo, sums)) is None   # the two registries do not answer for each other


def test_functional_re_exports_the_moved_names():
    for name in ("publish_t_copy", "t_copy_of", "publish_fwd3", "fwd3_of", "publish_grad3", "grad3_of", "grad3_decode", "publish_rows", "take_rows",
                 "zero_sums", "linear_chain", "hook_free", "set_grad_resid3", "grad_resid3_enabled", "_g3_partner_feeds"):
        assert getattr(UF, name) is getattr(handoff, name), name
    assert UF.clear_t_copies is handoff.clear
    assert not {"chain_depth", "fwd3_next_plain", "grad_resid3"} & set(UF._STATE)


# ------------------------------------------------------------------------------------------------ T copies
def _published(copy=None):
    g32 = torch.zeros(4, 6)
    g_t = torch.zeros(4, 6, dtype=BF16) if copy is None else copy
    UF.publish_t_copy(g32, g_t)
    return g32, g_t


def _is_miss(g32, dt, **kw):
    with pytest.raises(UiaError):                  # the miss path casts afresh, and ops.cast refuses CPU tensors
        UF.t_copy_of(g32, dt, **kw)
    return True


def test_a_published_t_copy_is_returned_once_as_that_object():
    g32, g_t = _published()
    assert UF.t_copy_of(g32, BF16) is g_t
    assert _is_miss(g32, BF16)                     # consumed


def test_fp32_asked_for_returns_the_input_and_leaves_the_entry():
    g32, g_t = _published()
    assert UF.t_copy_of(g32, torch.float32) is g32
    assert UF.t_copy_of(g32, BF16) is g_t


def test_an_fp32_copy_is_not_registered():
    g32 = torch.zeros(4, 6)
    UF.publish_t_copy(g32, g32)
    UF.publish_t_copy(g32, None)
    assert not handoff._T_COPIES


def test_a_write_after_publication_makes_the_t_copy_stale():
    g32, _ = _published()
    g32.add_(1.0)
    assert _is_miss(g32, BF16)


def test_another_view_at_the_same_address_does_not_get_the_t_copy():
    g32, _ = _published()
    assert g32.view(6, 4).data_ptr() == g32.data_ptr() and _is_miss(g32.view(6, 4), BF16)
    g32, _ = _published()
    assert _is_miss(g32.t(), BF16)                 # a transposed view


def test_another_dtype_asked_for_does_not_get_the_t_copy():
    g32, _ = _published()
    assert _is_miss(g32, torch.float16)


def test_a_k_blocked_t_copy_needs_allow_kb():
    kb = ops.KBlocked(torch.zeros(1, 4, ops.kb_group(BF16), dtype=BF16))
    g32, _ = _published(kb)
    assert _is_miss(g32, BF16)
    g32, _ = _published(kb)
    assert UF.t_copy_of(g32, BF16, allow_kb=True) is kb


def test_clear_drops_t_copies_and_the_registry_is_bounded():
    g32, _ = _published()
    UF.clear_t_copies()
    assert _is_miss(g32, BF16)
    keep = [_published() for _ in range(257)]
    assert len(handoff._T_COPIES) <= 256 and UF.t_copy_of(keep[-1][0], BF16) is keep[-1][1]


# ------------------------------------------------------------------------------------------------ rows hand-off and the row-sum arena
def _rows():
    return torch.zeros(4, 6), torch.zeros(4, 6, dtype=BF16), torch.zeros(4, 2, dtype=torch.int64)


def test_rows_left_on_a_stream_are_taken_once_on_that_stream():
    x32, x_t, sums = _rows()
    UF.publish_rows(x32, x_t, sums, stream=7)
    assert UF.take_rows(x32, BF16, stream=8) is None                           # another stream key
    got = UF.take_rows(x32, BF16, stream=7)
    assert isinstance(got, tuple) and got[0] is x_t and got[1] is sums
    assert UF.take_rows(x32, BF16, stream=7) is None                           # consumed


def test_rows_are_stale_after_a_write_and_not_for_a_non_contiguous_or_other_tensor():
    x32, x_t, sums = _rows()
    UF.publish_rows(x32, x_t, sums, stream=7)
    x32.mul_(2.0)
    assert UF.take_rows(x32, BF16, stream=7) is None                           # version
    xt32 = torch.zeros(6, 4).t()
    UF.publish_rows(xt32, x_t, sums, stream=7)
    assert not xt32.is_contiguous() and UF.take_rows(xt32, BF16, stream=7) is None
    UF.publish_rows(x32, x_t, sums, stream=7)
    assert UF.take_rows(x32[1:], BF16, stream=7) is None                       # another address
    UF.publish_rows(x32, x_t, sums, stream=7)
    assert UF.take_rows(x32, torch.float16, stream=7) is None                  # another dtype


def test_the_rows_hand_off_is_one_slot_per_stream():
    a, b = _rows(), _rows()
    UF.publish_rows(*a, stream=7)
    UF.publish_rows(*b, stream=7)
    assert UF.take_rows(a[0], BF16, stream=7) is None                          # overwritten ...
    assert UF.take_rows(b[0], BF16, stream=7) is None                          # ... and the failed lookup emptied the slot
    UF.publish_rows(*a, stream=7)
    UF.publish_rows(*b, stream=8)
    assert UF.take_rows(b[0], BF16, stream=8)[0] is b[1] and UF.take_rows(a[0], BF16, stream=7)[0] is a[1]
    UF.publish_rows(*a, stream=7)
    UF.clear_t_copies()
    assert UF.take_rows(a[0], BF16, stream=7) is None


def test_zero_sums_hands_out_the_slices_of_one_arena_per_stream_in_order():
    first, second, other = UF.zero_sums(5, CPU, stream=7), UF.zero_sums(5, CPU, stream=7), UF.zero_sums(5, CPU, stream=8)
    assert first.shape == (5, 2) and first.dtype == torch.int64 and not bool(first.any())
    arena = handoff._SUMS_ARENA[7][0]
    assert arena.shape == (48, 5, 2) and first.data_ptr() == arena[0].data_ptr() and second.data_ptr() == arena[1].data_ptr()
    assert other.data_ptr() == handoff._SUMS_ARENA[8][0].data_ptr() != arena.data_ptr()
    assert UF.zero_sums(9, CPU, stream=7).data_ptr() == handoff._SUMS_ARENA[7][0].data_ptr() != arena.data_ptr()      # another row count: a new arena
    for _ in range(47):
        UF.zero_sums(9, CPU, stream=7)
    full = handoff._SUMS_ARENA[7][0]
    assert UF.zero_sums(9, CPU, stream=7).data_ptr() == handoff._SUMS_ARENA[7][0].data_ptr() != full.data_ptr()      # all 48 handed out: a new arena


# ------------------------------------------------------------------------------------------------ K-blocked save / restore
def _kb():
    return ops.KBlocked(torch.zeros(1, 2, ops.kb_group(BF16), dtype=BF16))


@pytest.mark.parametrize("make, tag", [(lambda: torch.zeros(2, 32, dtype=BF16), "rows"), (_kb, "kb"),
                                       (lambda: handoff.Resid3(torch.zeros(2, 32, dtype=BF16), torch.zeros(2, 32, dtype=torch.int8)), "3rows"),
                                       (lambda: handoff.Resid3(_kb(), torch.zeros(2, 32, dtype=torch.int8)), "3kb")], ids=["tensor", "kb", "resid3", "resid3-kb"])
def test_save_and_restore_round_trip(make, tag):
    v = make()
    saved, tags = handoff.save_layout(v)
    assert tags == (tag,) and all(type(t) is torch.Tensor for t in saved) and len(saved) == (2 if isinstance(v, handoff.Resid3) else 1)
    (back,) = handoff.restore_layout(saved, tags)
    assert type(back) is type(v)
    hi, hi_back = (v.hi, back.hi) if isinstance(v, handoff.Resid3) else (v, back)
    assert type(hi_back) is type(hi) and (hi_back.t is hi.t if ops.is_kb(hi) else hi_back is hi)
    if isinstance(v, handoff.Resid3):
        assert back.lo is v.lo
    assert handoff.save_layout(back)[1] == tags


def test_save_and_restore_keep_the_order_of_a_mixed_list():
    import pickle
    x3, a, lse, x1 = handoff.Resid3(_kb(), torch.zeros(2, 32, dtype=torch.int8)), _kb(), None, torch.zeros(2, 32)
    saved, tags = handoff.save_layout(x3, a, lse, x1)
    assert tags == ("3kb", "kb", "rows", "rows") and len(saved) == 5 and pickle.loads(pickle.dumps(tags)) == tags
    b3, ba, blse, b1 = handoff.restore_layout(tuple(saved), tags)
    assert b3.hi.t is x3.hi.t and b3.lo is x3.lo and ba.t is a.t and blse is None and b1 is x1
