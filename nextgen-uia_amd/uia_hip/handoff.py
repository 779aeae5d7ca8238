"""Hand-offs that carry tensors BESIDE autograd between the Functions of a frozen tower (uia_hip.functional re-exports every name):

  T copies of fp32 gradients       publish_t_copy / t_copy_of     data pointer + version + storage, 256 deep
  three-byte gradient tokens       publish_grad3 / grad3_of       token address, pool of 64
  three-byte forward tokens        publish_fwd3 / fwd3_of         token address, pool of 256
  CLS-sparse gradient tokens       publish_cls_grad / cls_grad_of token address, pool of 64
  T rows + row sums (LN fold)      publish_rows / take_rows       raw stream, one slot
  zeroed row-sum arena             zero_sums                      raw stream, 48 slices
  "token 0 is all I read"          cls_only / take_cls_forward    one flag per call, consumed by the tower's head (CLS-only forward of the last layer)

with the rules that say when a token may be handed out (linear_chain, hook_free, _g3_partner_feeds, set_grad_resid3), the named type of a
three-byte value (Resid3), of a CLS-sparse gradient (ClsGrad) and the one place that knows how a K-blocked activation goes through save_for_backward (save_layout / restore_layout).
clear() drops all six channels.  Nothing here launches a kernel except the cast of a T copy that was not published, Resid3.decode() and ClsGrad.decode().
"""
from typing import NamedTuple

import torch

from . import ops

_STATE = {"chain_depth": 0, "fwd3_next_plain": False, "grad_resid3": False, "cls_grad": True,
          "cls_forward": True, "cls_decl": False, "cls_last": False, "cls_rows": False}


# ------------------------------------------------------------------------------------------------ three-byte values
class Resid3(NamedTuple):
    """A three-byte tensor (ops / include/uia_hip.h): the bf16 hi plane — the T copy itself, row-major or ops.KBlocked — plus one low byte per element.
    A tuple, so ops.gemm(resid3=), ops.layernorm_bwd(x= / dres=) and ops.mona_pre_bwd(dy=) take it as it is."""
    hi: object
    lo: torch.Tensor

    def decode(self):
        """fp32 values (slow path of a consumer that cannot take the planes: torch ops)."""
        return ops.three_byte_to_float(self.hi, self.lo).contiguous()


class Fwd3(NamedTuple):
    """A three-byte residual-stream VALUE on its way to the next block: the planes and the row sums (Σ, Σ²) of its rows for the folded LayerNorm."""
    hi: object
    lo: torch.Tensor
    sums: torch.Tensor

    @property
    def resid3(self):
        return Resid3(self.hi, self.lo)


class ClsGrad(NamedTuple):
    """A [B, N, D] residual-stream gradient that is zero outside token 0 of every image (the gradient a CLS-pooling head returns): the B non-zero rows in
    fp32 and, in bf16 mode, their T copy.  MonaFn.backward and VitBlockFn.backward run their row-wise stages on these rows alone."""
    rows32: torch.Tensor
    rows_t: object
    tokens: int

    def decode(self):
        """The dense fp32 [B, N, D] gradient: zeros plus a scatter (slow path of a consumer that cannot take the rows: torch ops)."""
        B, D = self.rows32.shape
        dense = self.rows32.new_zeros(B, self.tokens, D)
        dense[:, 0] = self.rows32
        return dense


def save_layout(*values):
    """(tensors for ctx.save_for_backward, layout tags) of activations that are a tensor, an ops.KBlocked or a Resid3 of either: save_for_backward
    takes tensors only, so a K-blocked wrapper is saved as its `.t` and a Resid3 as its two planes; restore_layout() rebuilds them from the tags."""
    tensors, tags = [], []
    for v in values:
        three = isinstance(v, Resid3)
        hi = v.hi if three else v
        kb = ops.is_kb(hi)
        tensors.append(hi.t if kb else hi)
        if three:
            tensors.append(v.lo)
        tags.append(("3" if three else "") + ("kb" if kb else "rows"))
    return tensors, tuple(tags)


def restore_layout(tensors, tags):
    it, out = iter(tensors), []
    for tag in tags:
        hi = next(it)
        if tag.endswith("kb"):
            hi = ops.KBlocked(hi)
        out.append(Resid3(hi, next(it)) if tag[0] == "3" else hi)
    return out


# ------------------------------------------------------------------------------------------------ tokens
class TokenRegistry:
    """autograd wants a tensor of the value's shape where a three-byte one travels: it gets a TOKEN — one NaN float expanded to that shape, no memory —
    and the payload travels here under the token's address.  Anything but take() that reads a token reads NaN: a topology the hand-off does not
    cover fails loudly, not quietly.  `size`: slots of the per-device ring of NaNs (consecutive tokens differ in address) and bound of the registry."""

    def __init__(self, size):
        self.size, self._pools, self._live = size, {}, {}

    def publish(self, shape, device, payload):
        key = (device.type, device.index if device.index is not None else (torch.cuda.current_device() if device.type == "cuda" else 0))
        pool = self._pools.get(key)
        if pool is None:
            pool = self._pools[key] = [torch.full((self.size,), float("nan"), device=device, dtype=torch.float32), 0]
        i = pool[1]
        pool[1] = (i + 1) % self.size
        tok = pool[0][i:i + 1].view((1,) * len(shape)).expand(shape)
        if len(self._live) >= self.size:
            self._live.clear()
        self._live[tok.data_ptr()] = (payload, tok.numel())
        return tok

    def take(self, t):
        """The payload when t is a token of publish() seen through views (consumed), else None.  Call BEFORE anything touches t's values
        (t.contiguous() would materialise NaNs)."""
        if not self._live or t.dim() == 0 or any(st != 0 for st, n in zip(t.stride(), t.shape) if n > 1):      # (a dimension of size 1 keeps whatever stride it had: a one-image slice)
            return None
        payload, numel = self._live.pop(t.data_ptr(), (None, 0))
        return payload if numel == t.numel() else None

    def clear(self):
        self._live.clear()


# THREE-BYTE residual gradients between the backward Functions of a frozen tower (round 4).  The fp32 gradient of the residual stream is
# written by one row kernel (4 B + its 2-byte T copy) and read back by the next (4 B), three times per layer; as a three-byte tensor the same
# hand-off is 3 B written and 3 B read.  Only MonaFn and VitBlockFn produce and consume tokens, and a producer hands one out only when its
# forward saw that the tensor it is the gradient of came straight (through views) from the other Function (so the token's only reader is
# that Function's backward).  Opt-in per step (set_grad_resid3; engine.contrastive_step turns it on for hook-free towers).
GRAD3 = TokenRegistry(64)
# Forward twin: a residual-stream VALUE handed from MonaFn to the next block's VitBlockFn as (hi plane, low bytes, row sums).
FWD3 = TokenRegistry(256)
# A CLS-sparse gradient from the head to the last adapter / block of a tower, and from that adapter to the block in front of it (ClsGrad).
CLSG = TokenRegistry(64)
_G3_VIEWS = ("PermuteBackward0", "ViewBackward0", "UnsafeViewBackward0", "TransposeBackward0", "AliasBackward0", "ReshapeAliasBackward0")
_G3_PARTNERS = ("MonaFnBackward", "VitBlockFnBackward")


def publish_grad3(shape, device, hi, lo):
    """Register the planes of a three-byte gradient and return the token autograd carries in its place."""
    return GRAD3.publish(shape, device, Resid3(hi, lo))


def grad3_of(g):
    """Resid3(hi, lo) when g is a token of publish_grad3 (consumed), else None.  Call BEFORE anything touches g's values."""
    return GRAD3.take(g)


def grad3_decode(hi, lo):
    return Resid3(hi, lo).decode()


def publish_fwd3(shape, device, hi, lo, sums):
    return FWD3.publish(shape, device, Fwd3(hi, lo, sums))


def fwd3_of(x):
    """Fwd3(hi, lo, sums) when x is a token of publish_fwd3 (consumed), else None.  Call BEFORE anything touches x's values."""
    return FWD3.take(x)


def publish_cls_grad(shape, device, rows32, rows_t):
    """Register the CLS rows of a gradient of `shape` = [B, N, D] and return the token autograd carries in its place."""
    return CLSG.publish(shape, device, ClsGrad(rows32, rows_t, shape[1]))


def cls_grad_of(g):
    """ClsGrad when g is a token of publish_cls_grad (consumed), else None.  Call BEFORE anything touches g's values."""
    return CLSG.take(g)


def set_cls_grad(flag):
    """Switch of the CLS-sparse backward (default on; off: the head hands on the dense gradient it always did).  It only ever applies where three-byte gradient
    tokens may travel: the per-step opt-in set_grad_resid3 is on and the head's input comes straight from a MonaFn / VitBlockFn."""
    _STATE["cls_grad"] = bool(flag)


def cls_grad_enabled():
    return _STATE["cls_grad"] and _STATE["grad_resid3"]


def set_grad_resid3(flag):
    _STATE["grad_resid3"] = bool(flag)


def grad_resid3_enabled():
    return _STATE["grad_resid3"]


class linear_chain:
    """Scope of a tower's own block loop (forward_features / VisionTransformer.forward): inside it the residual stream is a plain chain block -> adapter -> block,
    every block output has exactly ONE consumer, so a three-byte gradient token can stand in for its gradient.  Code that walks the blocks itself and taps
    intermediate outputs (FPN heads, CLIPSeg's extract layers) never enters the scope and gets fp32 residual gradients (a token with a second
    consumer would be ADDED to a real gradient by autograd)."""

    def __enter__(self):
        _STATE["chain_depth"] += 1
        return self

    def __exit__(self, *exc):
        _STATE["chain_depth"] -= 1
        _STATE["fwd3_next_plain"] = False
        _STATE["cls_last"] = _STATE["cls_rows"] = False
        return False

    @staticmethod
    def last_block_cls(flag):
        """The tower's loop says, before it runs a block, whether it is the LAST one, plain frozen and hook-free, under a head that reads token 0 only
        (take_cls_forward): that block — and the adapter behind it — may then compute the B CLS rows of its output and nothing else."""
        _STATE["cls_last"] = bool(flag)

    @staticmethod
    def next_is_plain_block(flag):
        """The tower's loop says, before it runs block i, whether block i + 1 exists and is a plain frozen block (VitBlockFn): only then may block i's adapter hand its
        output over as a three-byte forward token (set_fwd_resid3)."""
        _STATE["fwd3_next_plain"] = bool(flag)


def fwd3_consumer_ahead():
    """Inside a tower's own block loop, and the loop said that a plain frozen block comes next."""
    return _STATE["fwd3_next_plain"] and _STATE["chain_depth"] > 0


def take_last_block_cls():
    """True once, inside a tower's block loop whose head said that the last block may run on the CLS rows (consumed by that block's Function)."""
    flag = _STATE["cls_last"] and _STATE["chain_depth"] > 0
    _STATE["cls_last"] = False
    return flag


def cls_rows_out(flag):
    """A block that ran on the CLS rows says so: its output is [B, 1, D], and the adapter behind it takes that as the CLS rows of a [B, 1 + h·w, D] tensor."""
    _STATE["cls_rows"] = bool(flag)


def take_cls_rows():
    flag = _STATE["cls_rows"] and _STATE["chain_depth"] > 0
    _STATE["cls_rows"] = False
    return flag


class cls_only:
    """Per-call declaration of a tower's CALLER: "I read token 0 of this tower's output and nothing else" — what a contrastive step does with both towers.
    The tower's head consumes it (take_cls_forward) on its way in, so a nested tower call of another consumer never sees it, and the scope's exit clears
    it whether the call returned or raised.  Without it (a bare encode_image / encode_text, forward_features for a dense head) every layer runs dense."""

    def __enter__(self):
        _STATE["cls_decl"] = True
        return self

    def __exit__(self, *exc):
        _STATE["cls_decl"] = False
        return False


def take_cls_forward():
    """The declaration of cls_only(), consumed; False when the global switch set_cls_forward is off."""
    flag = _STATE["cls_decl"] and _STATE["cls_forward"]
    _STATE["cls_decl"] = False
    return flag


def cls_declared():
    return _STATE["cls_decl"]


def set_cls_forward(flag):
    """Switch of the CLS-only forward of a tower's last layer (default on; off: the dense launches, for A/B).  It only ever applies under cls_only()."""
    _STATE["cls_forward"] = bool(flag)


def hook_free(*modules):
    """No forward / forward-pre / backward hook on any of the modules or their submodules, and no global module hook: nothing but the towers' own Functions
    reads the tensors handed between them.  A three-byte forward token is a stride-0 NaN placeholder to everyone but its consumer (an activation
    tap or Grad-CAM hook on a block would read NaNs; a hook that returns a new tensor would feed them into the next block)."""
    import torch.nn.modules.module as _mm
    if _mm._global_forward_hooks or _mm._global_forward_pre_hooks or _mm._global_backward_hooks or getattr(_mm, "_global_backward_pre_hooks", None) \
            or getattr(_mm, "_global_forward_hooks_always_called", None):
        return False
    for mod in modules:
        for m in mod.modules():
            if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None):
                return False
    return True


def partner_node(x, in_chain=True):
    """The backward node of the MonaFn / VitBlockFn whose output x is, seen through view nodes only (the gradient a Function returns for x goes to that node's
    backward and nowhere else), or None.  in_chain = False: the caller runs behind the tower's block loop (the CLS head: linear_chain has closed by then)."""
    if not _STATE["grad_resid3"] or (in_chain and _STATE["chain_depth"] <= 0):
        return None
    fn = x.grad_fn
    for _ in range(8):
        if fn is None:
            return None
        name = type(fn).__name__
        if name in _G3_PARTNERS:
            return fn
        if name not in _G3_VIEWS or len(fn.next_functions) != 1:
            return None
        fn = fn.next_functions[0][0]
    return None


def _g3_partner_feeds(x):
    """True when x is the output of a MonaFn / VitBlockFn seen through view nodes only: the gradient this Function returns for x goes to that Function's backward."""
    return partner_node(x) is not None


def takes_cls_grad(x, in_chain=True):
    """True when the gradient returned for x may be a ClsGrad token: the switch and the per-step opt-in are on, x comes straight from a MonaFn / VitBlockFn, and
    that Function's forward said (ctx.cls_ok) that its backward runs on the CLS rows."""
    return cls_grad_enabled() and bool(getattr(partner_node(x, in_chain), "cls_ok", False))


# ------------------------------------------------------------------------------------------------ T copies
# T copies of fp32 gradient tensors travel beside autograd: the kernel that produces a residual
# gradient also writes its T copy (operand of the consumer's first dgrad GEMM); the consumer looks
# it up by storage address instead of re-reading 4 bytes/element to cast.
_T_COPIES = {}


def publish_t_copy(g32, g_t):
    """The entry keeps a STRONG reference to the fp32 gradient: while it is registered its storage cannot be freed, so no
    later tensor can appear at the same address and pick up a stale copy (a registry keyed by address alone did exactly that
    when two backward passes ran without clear_t_copies() in between).  Entries are consumed by the first lookup; the
    training loops clear what was never looked up once per step, and the registry is bounded besides."""
    if g_t is not None and g_t.dtype != torch.float32:
        if len(_T_COPIES) >= 256:
            _T_COPIES.clear()
        _T_COPIES[g32.data_ptr()] = (g32, g32._version, g_t)


def t_copy_of(g32, dt, allow_kb=False):
    """Return a T copy of the fp32 gradient `g32` (the one its producer published, if it is still that tensor's content).
    allow_kb: the caller feeds the copy to a ring GEMM as its A operand and nothing else, so a K-blocked copy (3-D, ops.kb_empty) will do;
    every other caller gets a row-major [.., D] tensor (a K-blocked publication is ignored and the copy is cast afresh)."""
    if dt == torch.float32:
        return g32
    hit = _T_COPIES.pop(g32.data_ptr(), None)
    if hit is not None:
        src, version, g_t = hit
        if (src.shape == g32.shape and src.stride() == g32.stride() and version == g32._version
                and src.untyped_storage().data_ptr() == g32.untyped_storage().data_ptr() and g_t.dtype == dt and (allow_kb or not ops.is_kb(g_t))):
            return g_t
    out = torch.empty(g32.shape, device=g32.device, dtype=dt)
    ops.cast(g32.contiguous(), out)
    return out


# ------------------------------------------------------------------------------------------------ row sums and rows of a folded LayerNorm
# Zeroed [M, 2] row-sum buffers for the producers of folded LayerNorms: slices of one arena that a single fill zeroes (a block needs two or
# three of them per forward; 36 fills of 400 KB per step otherwise).  A slice is handed out once; the arena is dropped with the other
# per-step registries (clear) or when it runs out, and a new one is zeroed on the next request.  One arena per STREAM: the fill
# that zeroes it and the atomics that land in its slices are ordered by that stream only (contrastive_step(overlap_text=True) runs the
# text tower on a second stream; a shared arena would hand it slices with no event between the fill and their first use).
# `stream` (here and in the rows hand-off): the key, ops.raw_stream() of the current stream unless the caller names one (host tests have no device).
_SUMS_ARENA = {}


def zero_sums(M, device, stream=None):
    key = ops.raw_stream() if stream is None else stream
    a = _SUMS_ARENA.get(key)
    if a is None or a[0].shape[1] != M or a[0].device != device or a[1] >= a[0].shape[0]:
        a = [torch.zeros(48, M, 2, device=device, dtype=torch.int64), 0]
        _SUMS_ARENA[key] = a
    a[1] += 1
    return a[0][a[1] - 1]


# The forward twin of the T copies, one slot deep: the GEMM that produces a residual-stream tensor (Mona project2, a block's fc2)
# can leave the T copy of its rows and their (Σ, Σ²) for the LayerNorm folded into the next block's first GEMM.
_ROWS = {}          # one slot per stream (the producer and the consumer of a hand-off run on the same stream)


def publish_rows(x32, x_t, sums, stream=None):
    _ROWS[ops.raw_stream() if stream is None else stream] = (x32, x32._version, x_t, sums)


def take_rows(x32, dt, stream=None):
    hit = _ROWS.pop(ops.raw_stream() if stream is None else stream, None)
    if hit is not None:
        src, version, x_t, sums = hit
        if (src.data_ptr() == x32.data_ptr() and src.numel() == x32.numel() and version == x32._version
                and src.untyped_storage().data_ptr() == x32.untyped_storage().data_ptr() and x32.is_contiguous() and x_t.dtype == dt):
            return x_t, sums
    return None


def clear():
    """Drops what the five channels still hold (the training loops: once per step).  functional.clear_t_copies is this."""
    _T_COPIES.clear()
    _ROWS.clear()
    _SUMS_ARENA.clear()
    GRAD3.clear()
    FWD3.clear()
    CLSG.clear()
