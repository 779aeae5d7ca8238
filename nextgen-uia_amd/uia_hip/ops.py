"""Tensor-level wrappers over the C ABI: torch tensors in, kernels launched on the current stream.

PyTorch is only plumbing here (device memory, streams); there is no arithmetic in this file and no
CPU path: CPU tensors raise.  `dtype` of an op is taken from its operand tensors
(torch.bfloat16 -> UIA_BF16, torch.float32 -> UIA_F32).
"""
import ctypes as C
from typing import NamedTuple

import torch

from . import _lib
from ._lib import AttnDesc, GemmDesc, LnLoraDesc, LoraRankDesc, MonaFusedDesc, MonaSpatialDesc, PackDesc, UiaError, WgradGroupDesc, check, lib

_ACT = {None: 0, "none": 0, "gelu": 1, "quick_gelu": 2, "relu": 3}

# When set to a list, every uia_gemm launch is bracketed by two events on the launch stream and
# (start, end, M, N, K, dtype, tile_cfg) is appended: bench.py's live per-kernel roofline measurement.
GEMM_PROFILE = None


EPI_BIAS, EPI_AUX_OUT, EPI_GELU, EPI_DGELU, EPI_RESID, EPI_RESIDT, EPI_OUT32, EPI_OUTT, EPI_RESID_LN, EPI_GENERIC = 1, 2, 4, 8, 16, 32, 64, 128, 256, -1
EPI_QUICK = 2048
EPI_ROWSUM, EPI_LNFOLD = 512, 1024
EPI_RESID_LO, EPI_OUT_LO = 4096, 8192      # three-byte tensors (bf16 hi plane + signed low byte): uia_gemm_desc.resid_lo8 / out_lo8
_SPECIALISED = {EPI_BIAS | EPI_RESID | EPI_OUT32, EPI_BIAS | EPI_RESIDT | EPI_OUT32, EPI_BIAS | EPI_RESID | EPI_RESID_LN | EPI_OUT32, EPI_OUTT, EPI_BIAS | EPI_OUTT, EPI_BIAS | EPI_GELU | EPI_OUTT, EPI_DGELU | EPI_OUTT,
                EPI_BIAS | EPI_GELU | EPI_AUX_OUT | EPI_OUTT,
                EPI_QUICK | EPI_BIAS | EPI_GELU | EPI_OUTT, EPI_QUICK | EPI_DGELU | EPI_OUTT, EPI_QUICK | EPI_BIAS | EPI_GELU | EPI_AUX_OUT | EPI_OUTT,
                EPI_BIAS | EPI_RESID | EPI_OUT32 | EPI_OUTT | EPI_ROWSUM, EPI_BIAS | EPI_RESID | EPI_RESID_LN | EPI_OUT32 | EPI_OUTT | EPI_ROWSUM,
                EPI_BIAS | EPI_OUTT | EPI_LNFOLD, EPI_BIAS | EPI_GELU | EPI_OUTT | EPI_LNFOLD, EPI_BIAS | EPI_GELU | EPI_AUX_OUT | EPI_OUTT | EPI_LNFOLD,
                EPI_QUICK | EPI_BIAS | EPI_GELU | EPI_OUTT | EPI_LNFOLD, EPI_QUICK | EPI_BIAS | EPI_GELU | EPI_AUX_OUT | EPI_OUTT | EPI_LNFOLD,
                EPI_BIAS | EPI_RESID_LO | EPI_RESID_LN | EPI_OUTT | EPI_OUT_LO | EPI_ROWSUM,
                EPI_BIAS | EPI_RESID | EPI_OUTT | EPI_OUT_LO | EPI_ROWSUM, EPI_BIAS | EPI_RESID_LO | EPI_OUT32,
                EPI_BIAS | EPI_RESID | EPI_RESID_LN | EPI_OUTT | EPI_OUT_LO | EPI_ROWSUM, EPI_BIAS | EPI_RESID_LO | EPI_RESID_LN | EPI_OUT32,
                EPI_BIAS | EPI_RESID_LO | EPI_OUT32 | EPI_OUTT | EPI_ROWSUM}

# the masks csrc/gemm_quad.hip instantiates (tile cfg 25); the rest run its run-time epilogue
_QUAD_SPECIALISED = _SPECIALISED - {EPI_BIAS | EPI_RESIDT | EPI_OUT32, EPI_BIAS | EPI_RESID | EPI_RESID_LN | EPI_OUT32, EPI_BIAS | EPI_RESID | EPI_RESID_LN | EPI_OUT32 | EPI_OUTT | EPI_ROWSUM,
                                    EPI_BIAS | EPI_RESID | EPI_RESID_LN | EPI_OUTT | EPI_OUT_LO | EPI_ROWSUM, EPI_BIAS | EPI_RESID_LO | EPI_RESID_LN | EPI_OUT32,
                                    EPI_BIAS | EPI_RESID_LO | EPI_OUT32 | EPI_OUTT | EPI_ROWSUM}


def epi_mask_of(d):
    """Mirror of epi_mask_of() in csrc/gemm.hip: the compile-time epilogue instantiation a descriptor lands on."""
    if d.alpha != 1.0 or d.out_group > 0 or d.resid_mod > 0:
        return EPI_GENERIC
    gl = (_ACT["gelu"], _ACT["quick_gelu"])
    if (d.act and d.act not in gl) or (d.dact and d.dact not in gl) or (d.act and d.dact and d.act != d.dact):
        return EPI_GENERIC
    quick = _ACT["quick_gelu"] in (d.act, d.dact)
    m = ((EPI_QUICK if quick else 0) | (EPI_BIAS if d.bias else 0) | (EPI_AUX_OUT if d.aux_out else 0) | (EPI_GELU if d.act else 0) | (EPI_DGELU if d.dact else 0) |
         (EPI_RESID if d.resid else 0) | (EPI_RESIDT if (d.residT and not d.resid_lo8) else 0) | (EPI_OUT32 if d.out32 else 0) | (EPI_OUTT if d.outT else 0) |
         (EPI_RESID_LN if ((d.resid or d.resid_lo8) and d.resid_ln_stats) else 0) | (EPI_ROWSUM if d.rowsum_out else 0) | (EPI_LNFOLD if d.lnfold_sums else 0) |
         (EPI_RESID_LO if d.resid_lo8 else 0) | (EPI_OUT_LO if d.out_lo8 else 0))
    return m


def auto_tile_cfg(M, N, K=None, esz=2, mask=EPI_GENERIC):
    """Mirror of launch_typed() in csrc/gemm.hip (which kernel instantiation a shape runs on)."""
    if N <= 64:
        stream64 = N == 64 and M > 2048 and esz == 2 and K is not None and K % 32 == 0 and 64 * (2 * K + 16) <= 160 * 1024
        if stream64 and mask in (EPI_OUTT, EPI_BIAS | EPI_OUTT, EPI_GENERIC):      # EPI_GENERIC = not known yet (the first look, before the descriptor is filled)
            return 16
        return 14 if (M > 2048 and esz == 2 and K is not None and K >= 1024) else 4
    if M <= 2048:
        return 21 if (esz == 4 and ((M + 127) // 128) * ((N + 127) // 128) < 64) else 3
    if K is not None and K * esz <= 128:
        return 14
    return 8


RING_CFGS = (8, 9, 10, 12, 13, 14, 24, 25, 26, 27, 28, 29)
PERSIST_STORE_ONLY = False   # experiment knob: 256x256 ring launches whose epilogue only stores T results run on the persistent variant (cfg 12)
KBLOCK_W = True          # hand the ring kernels their weights K-blocked (PackedW.kblocked()); False = row-major everywhere
K64_CFG14 = True         # single-K-step GEMMs on the two-workgroups-per-CU half-height config (False: 256x256 like every other large shape)
TILE_GROUP = {}          # experiment knob: {N: row panels per tile-order group} overriding the launcher's choice for ring launches with that N
SHORT_K_WIDE_HALF_STASH = True   # ... also for launches that write a second output (fc1 with the pre-activation stash)
SHORT_K_WIDE_HALF_BYTES = 2048   # ... and the longest K row (bytes) it applies to (fc1 of ViT-B: 1536, of ViT-L/14: 2048)
SHORT_K_WIDE_HALF_N = 3072   # N at and above which a short-K (K row <= SHORT_K_WIDE_HALF_BYTES) bf16 launch runs wholly on half-height tiles, two workgroups per CU (cfg 14); 0 = off (bench.py --short-k-half-n)
HALF_HEIGHT_SHORT_K_ALWAYS = False   # experiment knob: ... also when the 256-row tiling has no ragged last round (the text tower's N = 768, K = 768 sums at 65 536 rows)
HALF_HEIGHT_SHORT_K = True   # N <= 768, K <= 768 (bf16) launches whose 256-row tiling leaves a ragged last round run on half-height tiles (cfg 14) in one launch
CHAINS = 1               # independent chains of launches the caller has in flight on different streams (engine.contrastive_step sets it for the step): > 1 relaxes TAIL_SPLIT
TAIL_SPLIT = True        # split off the M tail of a launch whose last round of 256x256 tiles would leave most CUs idle
TAIL_SIDE_STREAM = True  # a SMALL M tail (at most a quarter of the CUs' worth of half-height tiles) runs on a side stream beside the main launch instead of behind it
MONA_PRE_FWD_T = True    # Mona forward: project1 (768 -> 64) inside the pre-norm row kernel (uia_mona_pre_fwd_t) instead of the N = 64 stream launch reading u back
MONA_PRE_BWD_DU = True   # Mona backward: project1's data gradient (K = 64) inside the pre-norm backward row kernel (uia_mona_pre_bwd_du) instead of a GEMM launch + a 77 MB round trip
LN_LORA_DOWN = True      # LoRA block: LayerNorm and the q / k / v down-projections drop_i(h)·A_iᵀ in one launch (uia_ln_lora_down) instead of the LayerNorm kernel + three N = 64 launches reading h back
LORA_REGEN_DROP = True   # LoRA input dropout: the forward does not write the dropped rows; the dA weight-gradient launch regenerates the mask while it stages x (uia_wgrad_drop)
LORA_RANK3 = True        # q | k | v of a LoRA block: the three rank terms of the data gradient in one pass over it (uia_lora_rank_update) instead of three K = 64 launches
QUAD = False             # 256x256 bf16 launches on the four-wave kernel (tile cfg 25, csrc/gemm_quad.hip: 128 x 128 per wave, one wave per SIMD) instead of cfg 8
QUADV = False            # experiment knob: 256x256 bf16 launches on the four-wave register-staged kernel (tile cfg 27, csrc/gemm_quadv.hip) instead of cfg 8
RING5 = False            # experiment knob: 256x256 launches with a long K loop or a wide N on the 5-deep ring (tile cfg 24: 160 KB of LDS, four sub-tiles in flight)
LORA_KEXT = True         # LoraAttnHalfFn: the rank update inside the frozen GEMM's K loop (uia_gemm_desc.A2 / K2) instead of a read-modify-write launch of its own
TAIL_SPLIT_K = True      # ... and run that tail split over K when it is a few tiles with a long K chain (two launches: slice partials, then sum + epilogue).
                         # Its slices meet through hardware float atomics: the rows of such a tail (<= 1/4 of the CUs busy: the ViT-L/14 + LoRA step, not the
                         # headline) vary in the last bit from run to run; set_deterministic(True) in functional turns it off.
_SPLITK_WS = {}
_TRACE_GENERIC = {} if __import__("os").environ.get("UIA_TRACE_GENERIC") else None
_TAIL_SIDE = {}
_NCU = {}


def num_cus(device=None):
    dev = torch.cuda.current_device() if device is None else device
    if dev not in _NCU:
        _NCU[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
    return _NCU[dev]


def big_tile_cfg(N, K, esz):
    """8 or 24 for a launch auto_tile_cfg() puts on the 256x256 ring tiles.  Isolated, plain epilogue (tools/time_ring_depth.py) the fifth ring slot is
    worth 4-5.5 % at K = 3072 and at 43 520 rows and 0.5-1.6 % at 65 536 x {2304, 3072} x 768 (and costs 7 % at N = 768, K = 768); inside the step, behind the
    fused epilogues, it is level to slightly worse on every one of those launches (44.5-44.9 ms either way, three alternating pairs on one box): opt-in."""
    if QUAD and esz == 2:
        return 25
    if QUADV and esz == 2:
        return QUADV if QUADV in (27, 29) else 27
    return 24 if (RING5 and esz == 2 and (K * esz >= 2048 or N >= 2304)) else 8


def tail_k_slices(rows, N, K, esz, ncu):
    """K slices for the half-height tail launch (tile cfg 13) of `rows` rows, or 0.  A tail of t tiles keeps t of the CUs busy for the whole K chain
    (ViT-L/14's 128-row tails: 4 tiles, 64 us at K = 4096); sliced over K it uses s·t CUs for 1/s of the chain, at the price of a second launch
    that sums the slices.  Worth it for at most a quarter of the CUs' worth of tiles and from 4 KiB of K per row; at least 1 KiB of K per slice."""
    tiles = -(-rows // 128) * -(-N // 256)
    kb = K * esz
    if not TAIL_SPLIT_K or esz != 2 or kb < 4096 or 4 * tiles > ncu:           # 81 tiles x 3 slices (the headline step's tails) measured level: the sum launch eats the gain
        return 0
    s = min(ncu // tiles, kb // 1024, 16)
    return s if s >= 2 else 0


def splitk_workspace(floats, device):
    """fp32 scratch of the split-K tail launches: one per (device, stream) — consecutive launches of a stream are ordered, two streams are not."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    t = _SPLITK_WS.get(key)
    if t is None or t.numel() < floats:
        t = _SPLITK_WS[key] = torch.zeros(max(floats, 1 << 20), device=device, dtype=torch.float32)     # zero once: the launches leave it zero
    return t


class _TailFork:
    """Fork / join around the tail launches of a split GEMM: `with fork:` enqueues on a side stream that starts where the caller's stream stands;
    fork.join() makes the caller's stream wait for it.  ViT-L/14 at 128 pairs has M = 128·257 rows: 128 full row panels (exactly two rounds of
    256 x 256 tiles at N = 1024) and ONE half panel, whose 4-16 tiles ran for 16 us per launch (x 2 with split K) BEHIND a 75-300 us main launch —
    pure latency, 2.3 ms per step.  Beside the main launch they cost a few CUs a few microseconds."""

    def __init__(self, device):
        self.cur = torch.cuda.current_stream(device)
        key = (device.index if device.index is not None else torch.cuda.current_device(), self.cur.cuda_stream)
        e = _TAIL_SIDE.get(key)
        if e is None:
            e = _TAIL_SIDE[key] = (torch.cuda.Stream(device=device), torch.cuda.Event(), torch.cuda.Event())
        self.side, self.ev_in, self.ev_out = e
        self.ctx = None

    def __enter__(self):
        self.ev_in.record(self.cur)
        self.side.wait_event(self.ev_in)
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self.ev_out.record(self.side)
        self.ctx.__exit__(*exc)
        return False

    def join(self):
        self.cur.wait_event(self.ev_out)


def small_tail(rows, N, ncu):
    """True when the tail of `rows` rows is few enough half-height tiles to run beside the main launch (TAIL_SIDE_STREAM)."""
    return TAIL_SIDE_STREAM and 4 * (-(-rows // 128) * -(-N // 256)) <= ncu


def drop_splitk_workspace(device):
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    _SPLITK_WS.pop(key, None)


def tail_split_rows(M, N, ncu, bm=256, bn=256):
    """Rows of the MAIN launch (a multiple of `bm`) when the 256x256 tiling should be split, else M.

    tiles = ceil(M/bm)·ceil(N/bn) workgroups run in rounds of `ncu`; when the last round holds at most half of the CUs
    (M = 50 432, N = 768: 591 = 2·256 + 79) its tiles are re-cut at half height (tile config 13, 128x256) so that they spread over
    twice as many CUs and the round takes about half as long: 2.55 instead of 3 tile times for that shape.  Pure scheduling —
    every output element is still one K-ordered fp32 accumulation, so results are identical to the unsplit launch."""
    tm, tn = -(-M // bm), -(-N // bn)
    tiles = tm * tn
    rem = tiles % ncu
    if tiles <= ncu or rem == 0 or 2 * rem > ncu:
        return M
    main_panels = (tiles - rem) // tn
    if main_panels < 1 or main_panels >= tm:
        return M
    return main_panels * bm


ROWSUM_SCALE = float(1 << 30)    # row sums (uia_gemm rowsum / lnfold / resid_ln with dim) are int64 fixed point in units of 2^-30: exact, order-free atomics


def rowsum_from_float(s):
    """fp32 [M, 2] (Σ, Σ²) -> the fixed-point form the kernels exchange (tests and host-side producers)"""
    return (s.double() * ROWSUM_SCALE).round().to(torch.int64).contiguous()


def rowsum_to_float(q):
    return (q.double() / ROWSUM_SCALE).float()


# Guard word of the folded LayerNorms (uia_gemm_desc.ln_flag): one zeroed int32 per device, handed to EVERY launch that writes or reads
# row sums, so every folded layer of every step is checked (on the device, at the cost of a compare per row) — not just the first few
# buffers of a warm-up step.  uia_hip.functional.poll_ln_flag() reads it back.
LN_FLAG_LIMIT = 8.0
_LN_FLAG = {}


def ln_flag(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    t = _LN_FLAG.get(key)
    if t is None:
        t = _LN_FLAG[key] = torch.zeros(1, device=device, dtype=torch.int32)
    return t


KBLOCK_ACT = True        # GEMM -> GEMM activations travel K-blocked ([K/g][rows][g]) between ring-kernel launches (kb_empty / is_kb)


def kb_group(dt):
    return 64 // dt.itemsize


def kb_ok(M, N_consumer, K, dt):
    """May an [M, K] activation that ONE GEMM epilogue writes and ONE GEMM (N_consumer columns) reads travel K-blocked?  Both launches
    must land on a ring tile config with 64-byte sub-tiles (M > 2048 and more than 64 columns on either side)."""
    return (KBLOCK_ACT and K % kb_group(dt) == 0 and K > 64 and auto_tile_cfg(M, N_consumer, K, dt.itemsize) in (8, 14)
            and auto_tile_cfg(M, K, 128, dt.itemsize) == 8)


class KBlocked:
    """An [M, K] activation stored K-blocked: `.t` is a [K/g, M, g] tensor (g = 64 bytes of elements; a row range `.t[:, lo:hi]` of a
    larger one is fine).  An explicit type rather than "any 3-D tensor": only ops.gemm (a / out_t) and the few producer kernels that
    were taught the layout accept it, everything else fails loudly on it."""
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t

    dtype = property(lambda self: self.t.dtype)
    device = property(lambda self: self.t.device)
    is_cuda = property(lambda self: self.t.is_cuda)
    rows = property(lambda self: self.t.shape[1])
    cols = property(lambda self: self.t.shape[0] * self.t.shape[2])

    def element_size(self):
        return self.t.element_size()

    def data_ptr(self):
        return self.t.data_ptr()

    def row_range(self, lo, hi):
        return KBlocked(self.t[:, lo:hi])

    def as_rows(self):
        """the same STORAGE as a row-major [M, K] buffer (contents are not converted: for re-use of a dead buffer)"""
        return self.t.reshape(-1).view(self.rows, self.cols)

    @staticmethod
    def over(buf):
        """the storage of a dead row-major [M, K] buffer as a K-blocked one (contents are not converted)"""
        g = kb_group(buf.dtype)
        M, K = buf.shape
        return KBlocked(buf.view(K // g, M, g))


def kb_empty(M, K, dt, device):
    g = kb_group(dt)
    return KBlocked(torch.empty(K // g, M, g, device=device, dtype=dt))


def is_kb(t):
    return isinstance(t, KBlocked)


def _kb_dims(kb, name):
    t = kb.t
    g = kb_group(t.dtype)
    if t.shape[2] != g or t.stride(2) != 1 or t.stride(1) != g or t.stride(0) % g or t.stride(0) // g < t.shape[1]:
        raise UiaError(f"{name}: not a K-blocked [K/{g}, rows, {g}] activation (shape {tuple(t.shape)}, stride {t.stride()})")
    return t.shape[1], t.shape[0] * g, t.stride(0) // g          # rows, columns, rows of the whole tensor (plane stride)


class Ready:
    """The stream that filled a cached device buffer and the event that orders every OTHER stream behind the fill (the weight
    caches are filled by whichever stream misses first; a hit from another stream — contrastive_step(streams=S), the text tower's side
    stream — launched GEMMs on a buffer whose cast / pack / transpose could still be in flight).  sync() is a set lookup on the filling
    stream and on every stream that has waited once."""
    __slots__ = ("event", "seen")

    def __init__(self):
        st = torch.cuda.current_stream()
        self.event = torch.cuda.Event()
        self.event.record(st)
        self.seen = {st.cuda_stream}

    def sync(self):
        rs = raw_stream()
        if rs not in self.seen:
            torch.cuda.current_stream().wait_event(self.event)
            self.seen.add(rs)


class PackedW:
    """A GEMM weight [N, K] in the compute dtype, with its K-blocked twin [K/g][N][g] (g = 64 bytes of elements) built on first
    use by a ring-kernel launch.  Layout plumbing only (a strided copy); which one a launch takes is decided in gemm().
    Construct it AFTER the kernels that fill `row` (and `kb`) were enqueued: it records the event other streams wait for."""
    __slots__ = ("_row", "_kb", "ready", "kb_ready")

    def __init__(self, row, kb=None):
        self._row, self._kb = row, kb
        self.ready = Ready() if row.is_cuda else None
        self.kb_ready = self.ready

    def refreshed(self, ready):
        """the buffers were rewritten in place (uia_pack_weights after an optimiser step)"""
        self.ready = self.kb_ready = ready

    @property
    def row(self):
        if self.ready is not None:
            self.ready.sync()
        return self._row

    @property
    def shape(self):
        return self._row.shape

    @property
    def dtype(self):
        return self._row.dtype

    @property
    def device(self):
        return self._row.device

    def kblocked(self):
        if self._kb is None:
            row = self.row                                       # orders this stream behind the fill of `row`
            N, K = row.shape
            g = 64 // row.element_size()
            self._kb = row.view(N, K // g, g).permute(1, 0, 2).contiguous()
            self.kb_ready = Ready() if row.is_cuda else None
        elif self.kb_ready is not None:
            self.kb_ready.sync()
        return self._kb


class ExtW:
    """A GEMM weight [N, K] that exists K-BLOCKED only ([K/g][N][g]) and whose last K2 columns pair with a second A operand (uia_gemm_desc.A2 / K2: the LoRA
    rank update inside the frozen GEMM).  Built by functional.WEIGHTS.get_lora_ext."""
    __slots__ = ("_kb", "N", "K", "K2", "ready", "__weakref__")

    def __init__(self, kb, N, K, K2):
        self._kb, self.N, self.K, self.K2 = kb, N, K, K2
        self.ready = Ready() if kb.is_cuda else None

    @property
    def kb(self):
        if self.ready is not None:
            self.ready.sync()
        return self._kb

    @property
    def device(self):
        return self._kb.device


class RawDest:
    """A uia_pack_weights destination that is a strided view inside a larger buffer (the kernel's rows_pad / cols_pad reproduce its strides)."""
    __slots__ = ("view",)

    def __init__(self, view):
        self.view = view


def gemm_kernel_name(cfg, mask, dtype):
    """(readable name, mangled fragment) of the instantiation a launch runs on.  rocprofv3 prints these kernels mangled
    (its demangler does not know the bf16 type code), so the fragment is what to grep for in profiles/*.csv."""
    m = mask if mask in _SPECIALISED else EPI_GENERIC
    tn, tc = ("bf16", "DF16b") if dtype == torch.bfloat16 else ("float", "f")
    mi = lambda v: f"Li{v}E" if v >= 0 else f"Lin{-v}E"
    if cfg == 12:
        return f"gemm_tn_persist_kernel<{tn},{m}>", f"gemm_tn_persist_kernelI{tc}{mi(m)}E"
    if cfg in (8, 13, 14, 24):
        bm, nbuf = (256, 4) if cfg == 8 else ((256, 5) if cfg == 24 else ((128, 4) if cfg == 13 else (128, 3)))
        return f"gemm_tn_ring_kernel<{tn},{bm},256,2,4,64,{nbuf},{m}>", "gemm_tn_ring_kernelI" + tc + "".join(mi(v) for v in (bm, 256, 2, 4, 64, nbuf, m, 0)) + "Lb0ELb0EE"
    if cfg in (25, 26):
        mq = m if (cfg == 25 and m in _QUAD_SPECIALISED) else EPI_GENERIC
        return f"gemm_tn_quad_kernel<{mq},false>", f"gemm_tn_quad_kernelI{mi(mq)}Lb0EE"
    if cfg == 29:
        mq = m if m in _QUAD_SPECIALISED else EPI_GENERIC
        return f"gemm_tn_quadvp_kernel<{mq}>", f"gemm_tn_quadvp_kernelI{mi(mq)}E"
    if cfg in (27, 28):
        mq = m if (m in _QUAD_SPECIALISED and (cfg == 27 or m == EPI_OUTT)) else EPI_GENERIC
        return f"gemm_tn_quadv_kernel<{mq},{cfg - 25},0>", f"gemm_tn_quadv_kernelI{mi(mq)}{mi(cfg - 25)}Li0EE"
    if cfg == 16:
        return "gemm_skinny64_kernel", "gemm_skinny64_kernel"
    if cfg == 23:
        return "gemm_wide64_kernel", "gemm_wide64_kernel"
    shape = {1: (256, 256, 2, 4), 2: (256, 128, 4, 2), 3: (128, 128, 2, 2), 4: (256, 64, 4, 1), 5: (128, 64, 2, 1), 21: (32, 64, 2, 2)}.get(cfg)
    if shape:
        return f"gemm_tn_kernel<{tn},{','.join(map(str, shape))}>", "gemm_tn_kernelI" + tc + "".join(mi(v) for v in shape) + "E"
    return f"tile cfg {cfg}", f"cfg{cfg}"


def _code(dt):
    if dt == torch.bfloat16:
        return _lib.BF16
    if dt == torch.float32:
        return _lib.F32
    raise UiaError(f"unsupported operand dtype {dt}")


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise UiaError("uia ops need CUDA/HIP tensors: there is no CPU fallback for the hot path")
    return t.data_ptr()


_HIP_OK = []


def raw_stream():
    """Handle of the current stream of the current device.  torch.cuda.current_stream() costs ~8 us of Python per call (device-index helpers, is_available, an
    os.environ lookup, a Stream object); every launch and every cached-weight hit asks — 390 times per CLIPSeg step, 3 ms of an 11 ms host-bound step.  Two C calls."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _stream():
    if not _HIP_OK:
        if not torch.cuda.is_available():
            raise UiaError("uia ops need an MI355X (HIP) device: there is no CPU fallback for the hot path")
        _HIP_OK.append(True)
    return raw_stream()


def _dense(t, name, dtypes, numel=None, align=1):
    """Refuse (UiaError, before any launch) an operand that is not a contiguous tensor of one of `dtypes` with exactly `numel`
    elements and a data pointer aligned to `align` bytes (the vector loads / stores of the kernel that reads it; "v4": four elements)."""
    if not isinstance(t, torch.Tensor):
        raise UiaError(f"{name}: a tensor is required, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise UiaError(f"{name}: dtype {t.dtype}, expected {' or '.join(str(d) for d in dtypes)}")
    if not t.is_contiguous():
        raise UiaError(f"{name}: must be contiguous (shape {tuple(t.shape)}, stride {t.stride()})")
    if numel is not None and t.numel() != numel:
        raise UiaError(f"{name}: {t.numel()} elements (shape {tuple(t.shape)}), expected {numel}")
    if align == "v4":
        align = 4 * t.element_size()
    if t.data_ptr() % align:
        raise UiaError(f"{name}: data pointer not aligned to {align} bytes")
    return t


def _require(cond, msg):
    if not cond:
        raise UiaError(msg)


_F32, _FT = (torch.float32,), (torch.bfloat16, torch.float32)


def _rowmajor(t, name):
    if t.dim() != 2 or t.stride(1) != 1:
        raise UiaError(f"{name} must be a 2-D row-major tensor (got shape {tuple(t.shape)}, stride {t.stride()})")
    return t.stride(0)


class Launch(NamedTuple):
    """One uia_gemm call of a planned gemm(): rows [lo, hi) of the problem."""
    lo: int
    hi: int
    tile_cfg: int       # the word uia_gemm receives: tile config (0 = the launcher's own choice) | rows per tile-order group << 8 | K slices << 16 | split-K phase << 22
    base: int           # the tile config the schedule counts on: tile_cfg's where it names one, else the mirror of the launcher's choice (auto_tile_cfg, 23)
    w_kblocked: bool    # the weight goes K-blocked
    side: bool          # enqueued on the side stream, beside the launches that are not (_TailFork)
    scratch: int        # fp32 elements of split-K scratch the launch works in (0: none)


def plan_gemm(M, N, K, esz, ncu, tile_cfg=0, *, whole=False, ext=False, packed=False, on_device=True, out_group=0, resid_mod=0, drop=None, alpha=1.0,
              a_kb=False, out_t_kb=False, act=False, aux_out=False, out_t=False, out32=False, resid=False, resid_t=False, rowsum=False, ln=False):
    """The uia_gemm launches of one gemm() call, in enqueue order: pure host logic over plain values and the module's knobs (no device, no tensor).

    M, N, K (an ExtW's whole K), esz = element size, ncu = compute units, tile_cfg = the caller's word.  Facts about the call: ext / packed = the weight is
    an ExtW / a PackedW; on_device; out_group, resid_mod, alpha as given; drop = None | "a" | "acc"; a_kb / out_t_kb = `a` / `out_t` travel K-blocked;
    act = act or dact given; ln = lnfold or resid_ln given; the rest = that operand is given.  whole = True plans what a direct _gemm_one call asks for:
    one launch of all rows on `tile_cfg`, none of the splitting below.

    With the launcher's own tile choice (tile_cfg == 0) the M tail of a launch whose last round of 256 x 256 tiles would leave most CUs idle goes through a
    launch of its own on half-height tiles (tail_split_rows; cfg 13), split over K in two phases when it is a few tiles with a long K chain (tail_k_slices),
    and beside the main launch (side stream, enqueued first) when it is small (small_tail), else behind it — or the whole launch moves to half-height
    tiles, two workgroups per CU (cfg 14)."""
    auto = 0 if (ext or tile_cfg & 255) else auto_tile_cfg(M, N, K, esz)

    def launch(lo, hi, word, side=False, scratch=0):
        base = word & 255
        if ext:
            if not base:            # W exists K-blocked only: ring tiles
                base = 8 if hi - lo > 2048 else 13
                word |= base
        elif not base:
            base = auto
            # mirror of wide64_ok() in csrc/gemm.hip: the K = 64 read-modify-write stream (LoRA rank update / its data gradient) takes row-major W
            if (base == 14 and esz == 2 and K == 64 and N % 64 == 0 and N * 144 <= 160 * 1024 and not (a_kb or out_t_kb or act or aux_out or rowsum or ln)
                    and out_group == 0 and resid_mod == 0 and drop in (None, "acc")
                    and ((out_t and not out32 and not resid and (resid_t or drop is not None)) or (out32 and not out_t and not resid_t and (resid or drop is not None)))):
                base = 23
            elif base == 8:
                base = big_tile_cfg(N, K, esz)
                word |= base
        if PERSIST_STORE_ONLY and base == 8 and not (resid or resid_t or out32 or rowsum) and out_group == 0 and alpha == 1.0 and K * esz >= 1024:
            base, word = 12, (word & ~255) | 12
        if TILE_GROUP and N in TILE_GROUP and (word >> 8) == 0 and base in RING_CFGS:
            word |= int(TILE_GROUP[N]) << 8
        return Launch(lo, hi, word, base, bool(ext or (packed and KBLOCK_W and base in RING_CFGS and on_device)), side, scratch)

    m_main = M
    if whole or not on_device:
        pass
    elif ext:
        if TAIL_SPLIT and tile_cfg == 0 and M > 2048:
            m_main = tail_split_rows(M, N, ncu)
    else:
        if not K64_CFG14 and tile_cfg == 0 and auto == 14:
            tile_cfg = 8
        if TAIL_SPLIT and tile_cfg == 0 and out_group == 0 and resid_mod == 0 and drop is None and auto == 8:
            m_main = tail_split_rows(M, N, ncu)
            if SHORT_K_WIDE_HALF_N and N >= SHORT_K_WIDE_HALF_N and K * esz <= SHORT_K_WIDE_HALF_BYTES and esz == 2 and (SHORT_K_WIDE_HALF_STASH or not aux_out):
                # short K loop, wide N (fc1 and its GELU' data gradient: K = 768, N = 3072): a quarter of a 256 x 256 launch is prologue + epilogue + hand-over that
                # nothing overlaps (profiles/r04_d); on half-height tiles two workgroups share a CU and one's seam runs beside the other's K loop:
                # 385 -> 338 us at M = 65 536, 266 -> 252 at 50 432 in isolation (bias + GELU store), level at N = 2304
                tile_cfg, m_main = 14, M
            if (m_main < M or HALF_HEIGHT_SHORT_K_ALWAYS) and HALF_HEIGHT_SHORT_K and CHAINS <= 1 and N <= 768 and K * esz <= 1536:      # (with other chains beside it a ragged round costs nothing: 40.99 -> 40.73 ms without this rule there)
                # short K loops with a ragged last round (the image tower's output projection and its data gradient: 591 tiles on 256 CUs): the whole
                # launch on half-height tiles, two workgroups per CU (tile cfg 14), instead of a main launch + a half-height tail launch — 1182 half
                # tiles pack 2.31 rounds of 512, and one workgroup's epilogue runs beside its neighbour's K loop (round 3, isolated: 64 vs 62 + 21 us
                # for the plain data gradient, 92 vs 102 us per 43 520 rows for the fp32-residual producer).  Longer K loops lose on it.
                tile_cfg, m_main = 14, M
    if m_main == M:
        return [launch(0, M, tile_cfg)]
    side = small_tail(M - m_main, N, ncu)
    if CHAINS > 1 and not side and not ext:
        # several independent chains of launches share the chip (engine.contrastive_step: the image tower in two slices beside the text tower): a ragged last
        # round is filled by the other chains' workgroups, and a tail launch BEHIND the main one only adds a launch (40.87 -> 40.70 ms).  Small tails still
        # fork to the side stream: without that split the ViT-L/14 + LoRA step loses 2.4 ms (a handful of tiles as a whole extra round).
        return [launch(0, M, tile_cfg)]
    slices = 0 if ext else tail_k_slices(M - m_main, N, K, esz, ncu)
    if slices:      # two phases: slice partials into the scratch, then sum + epilogue
        floats = -(-(M - m_main) // 128) * -(-N // 256) * 128 * 256
        tail = [launch(m_main, M, 13 | slices << 16 | phase << 22, side, floats) for phase in (1, 2)]
    else:
        tail = [launch(m_main, M, 13, side)]
    main = launch(0, m_main, 8 if ext else big_tile_cfg(N, K, esz))
    return tail + [main] if side else [main] + tail


def _plan_facts(a, w, act, dact, aux_out, out_group, resid_mod, drop, alpha, out_t, out32, resid, resid_t, rowsum, lnfold, resid_ln):
    """plan_gemm's keywords about a gemm() / _gemm_one() call"""
    return dict(ext=isinstance(w, ExtW), packed=isinstance(w, PackedW), on_device=a.is_cuda, out_group=out_group, resid_mod=resid_mod,
                drop=None if drop is None else drop[0], alpha=alpha, a_kb=is_kb(a), out_t_kb=is_kb(out_t), act=act is not None or dact is not None,
                aux_out=aux_out is not None, out_t=out_t is not None, out32=out32 is not None, resid=resid is not None, resid_t=resid_t is not None,
                rowsum=rowsum is not None, ln=lnfold is not None or resid_ln is not None)


def _cut(t, lo, hi, heads=1):
    """Rows [lo, hi) of a row-indexed gemm() operand: a tensor [M, ·] (an ExtW's grouped a2: [G, M, K2]), a
    KBlocked, None, or a tuple whose first `heads` elements are such operands and whose rest are parameters: (stats, …), (sums, …), (t2, group_cols);
    resid3 = (hi plane, low bytes) has two."""
    if t is None:
        return None
    if isinstance(t, tuple):
        return tuple(_cut(x, lo, hi) for x in t[:heads]) + tuple(t[heads:])
    if is_kb(t):
        return t.row_range(lo, hi)
    return t[lo:hi] if t.dim() < 3 else t[:, lo:hi]


def gemm(a, w, *, bias=None, act=None, dact=None, aux_in=None, aux_out=None, resid=None, resid_mod=0, resid_row_off=0,
         resid_t=None, out_group=0, out_t=None, out32=None, alpha=1.0, tile_cfg=0, resid_ln=None, rowsum=None, lnfold=None, drop=None, a2=None,
         resid3=None, out_lo=None):
    """C = epilogue(alpha * a @ w.T).  a [M,K], w [N,K] (tensor or PackedW) share a dtype (bf16 | fp32); see include/uia_hip.h.

    Host-side scheduling on top of uia_gemm (results do not depend on it): plan_gemm() says which launches the call becomes — with the automatic
    tile choice, a weight that came as a PackedW is handed to the ring kernels K-blocked, and the M tail of a launch whose last round of tiles would
    leave most CUs idle goes through a launch of its own on half-height tiles; this function cuts the operands and enqueues them.
    resid_ln = (stats [M, 2], ln_weight, ln_bias): `resid` is the INPUT of a LayerNorm whose output is the residual to add; a fourth and
    fifth element (dim, eps) say that `stats` holds the row sums (Σ, Σ²) a producing GEMM left through `rowsum`, not (mean, rstd).
    drop = ("a", p, seed[, a_drop_out]): LoRA input dropout applied to `a` in flight (N = 64 stream kernel only; a_drop_out receives the dropped
    rows), or ("acc", p, seed): applied to alpha·acc of element (m, n) before the residual adds — the generator of ops.dropout in both cases.
    rowsum = zeroed int64 [M, 2] (ROWSUM_SCALE fixed point; rowsum_to_float converts): receives (Σ, Σ²) of the stored fp32 rows.  lnfold = (sums [M, 2], colsum [N], dim, eps): `a` holds RAW
    rows and `w` is pre-scaled by the LayerNorm weight; the epilogue applies the LayerNorm (include/uia_hip.h, uia_gemm_desc).
    Three-byte tensors (bf16, ring tile configs: M > 2048): resid3 = (hi, lo) is the residual as a bf16 hi plane (row-major or KBlocked) plus an int8
    [M, N] plane of low bytes — float bits = (hi_bits << 16) + (lo << 8) — to which resid_ln then applies; out_lo = int8 [M, N] receives the low
    bytes of the result, whose hi plane is out_t (three_byte_to_float converts)."""
    if (resid3 is not None or out_lo is not None) and (isinstance(w, ExtW) or resid_mod or out_group or (a.t.dtype if is_kb(a) else a.dtype) != torch.bfloat16):
        raise UiaError("gemm: three-byte tensors (resid3 / out_lo) need bf16 operands and a plain epilogue (no row remapping, no K extension)")
    if isinstance(w, ExtW):
        # K extension: w = [W | s·B] (K-blocked only), a2 = (t, group_cols): t [M, K2] or [G, M, K2] — one [M, K2] operand per group of output columns
        if a2 is None or is_kb(a) or a.dtype != torch.bfloat16 or a.shape[1] != w.K - w.K2 or resid_mod or out_group or drop is not None:
            raise UiaError("gemm: an ExtW weight needs a2 = (t, group_cols), a row-major bf16 `a` of K - K2 columns and a plain epilogue")
        t2, gcols = a2
        M, N, K = a.shape[0], w.N, w.K
        if t2.dtype != a.dtype or t2.shape[-1] != w.K2 or t2.shape[-2] != M or t2.stride(-1) != 1 or t2.stride(-2) != w.K2 or (t2.dim() == 3 and t2.shape[0] * gcols != w.N):
            raise UiaError(f"gemm: a2 operand {tuple(t2.shape)} does not match [groups, {M}, {w.K2}] with {w.N} columns in groups of {gcols}")
    else:
        M, (N, K) = (a.rows if is_kb(a) else a.shape[0]), (w.row if isinstance(w, PackedW) else w).shape
    plan = plan_gemm(M, N, K, a.element_size(), num_cus(a.device.index) if a.is_cuda else 0, tile_cfg,
                     **_plan_facts(a, w, act, dact, aux_out, out_group, resid_mod, drop, alpha, out_t, out32, resid, resid_t, rowsum, lnfold, resid_ln))
    if len(plan) == 1:      # all rows at once: the operands pass as they came (row-remapped ones are not [M, ·])
        _gemm_one(a, w, bias=bias, act=act, dact=dact, aux_in=aux_in, aux_out=aux_out, resid=resid, resid_mod=resid_mod, resid_row_off=resid_row_off,
                  resid_t=resid_t, out_group=out_group, out_t=out_t, out32=out32, alpha=alpha, resid_ln=resid_ln, rowsum=rowsum, lnfold=lnfold, drop=drop,
                  a2=a2, resid3=resid3, out_lo=out_lo, launch=plan[0])
        return

    def run(launches):      # on whichever stream is current: the split-K scratch belongs to (device, stream)
        ws = None
        try:
            for L in launches:
                if L.scratch and ws is None:
                    ws = splitk_workspace(L.scratch, a.device)
                lo, hi = L.lo, L.hi
                _gemm_one(_cut(a, lo, hi), w, bias=bias, act=act, dact=dact, aux_in=_cut(aux_in, lo, hi), aux_out=_cut(aux_out, lo, hi), resid=_cut(resid, lo, hi),
                          resid_t=_cut(resid_t, lo, hi), out_t=_cut(out_t, lo, hi), out32=_cut(out32, lo, hi), alpha=alpha, resid_ln=_cut(resid_ln, lo, hi),
                          rowsum=_cut(rowsum, lo, hi), lnfold=_cut(lnfold, lo, hi), splitk_ws=ws if L.scratch else None, a2=_cut(a2, lo, hi),
                          resid3=_cut(resid3, lo, hi, 2), out_lo=_cut(out_lo, lo, hi), launch=L)
        except Exception:
            if ws is not None:      # phase 2 is what re-zeroes the shared scratch: an error between the two launches must not leave partial sums behind
                drop_splitk_workspace(a.device)
            raise

    side = [L for L in plan if L.side]
    if side:        # a small tail runs beside the main launch, not behind it
        fork = _TailFork(a.device)
        with fork:
            run(side)
        run([L for L in plan if not L.side])
        fork.join()
    else:
        run(plan)


def _plane(t, name, M, N, dtype, rows_checked=True):
    """An epilogue operand that covers the [M, N] result as a row-major tensor ([>= M, >= N]) or a KBlocked one ([>= M, N]) of `dtype`:
    (the tensor the kernel addresses, its row stride, the K-blocked plane stride in rows or 0)."""
    if is_kb(t):
        rows, cols, plane = _kb_dims(t, f"gemm {name}")
        if rows < M or cols != N or t.t.dtype != dtype:
            raise UiaError(f"gemm {name} (K-blocked {tuple(t.t.shape)} {t.t.dtype}) does not hold the [{M}, {N}] {dtype} plane")
        return t.t, N, plane
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] < N or (rows_checked and t.shape[0] < M):
        raise UiaError(f"gemm {name} is {tuple(t.shape)} {t.dtype}: it does not hold the [{M}, {N}] {dtype} plane")
    return t, _rowmajor(t, name), 0


def _gemm_one(a, w, *, bias=None, act=None, dact=None, aux_in=None, aux_out=None, resid=None, resid_mod=0, resid_row_off=0,
              resid_t=None, out_group=0, out_t=None, out32=None, alpha=1.0, tile_cfg=0, resid_ln=None, rowsum=None, lnfold=None, drop=None, splitk_ws=None, a2=None,
              resid3=None, out_lo=None, launch=None):
    """One uia_gemm launch: validate the operands, fill the descriptor, launch on `launch` (an entry of gemm()'s plan), or — called directly — on what
    plan_gemm makes of `tile_cfg` for one launch of all rows."""
    d = GemmDesc()
    if splitk_ws is not None:
        d.splitk_ws = _p(splitk_ws)
    ext = w if isinstance(w, ExtW) else None
    if ext is not None:
        t2, gcols = a2
        d.A2, d.lda2, d.K2 = t2.data_ptr(), t2.stride(-2), ext.K2
        d.a2_group_cols, d.a2_group_stride = (gcols, t2.stride(0)) if t2.dim() == 3 else (0, 0)
    if drop is not None:
        d.drop_where, d.drop_p, d.drop_seed = {"a": 1, "acc": 2}[drop[0]], float(drop[1]), int(drop[2]) & 0xFFFFFFFFFFFFFFFF
        if len(drop) > 3 and drop[3] is not None:
            xo = drop[3]
            if drop[0] != "a" or xo.dtype != a.dtype or xo.shape != a.shape or xo.stride() != a.stride():
                raise UiaError("gemm drop: a_drop_out must have a's dtype, shape and strides")
            d.a_drop_out = _p(xo)
    packed = w if isinstance(w, PackedW) else None
    if ext is not None:
        # W exists K-blocked only and spans K = (columns of a) + K2
        d.lda, d.ldw, d.M, d.K, d.N = _rowmajor(a, "a"), ext.K, a.shape[0], ext.K, ext.N
        d.A = _p(a)
    else:
        wrow = packed.row if packed is not None else w
        d.ldw = _rowmajor(wrow, "w")
        if is_kb(a):
            d.M, d.K, d.a_kb_rows = _kb_dims(a, "gemm a")
            d.lda = d.K
        else:
            d.lda = _rowmajor(a, "a")
            d.M, d.K = a.shape[0], a.shape[1]
        if a.dtype != wrow.dtype or d.K != wrow.shape[1]:
            raise UiaError(f"gemm operand mismatch: a {(d.M, d.K)} {a.dtype}, w {tuple(wrow.shape)} {wrow.dtype}")
        d.A = _p(a.t if is_kb(a) else a)
        d.N = wrow.shape[0]
    esz = a.element_size()
    if launch is None:
        launch = plan_gemm(d.M, d.N, d.K, esz, 0, tile_cfg, whole=True,
                           **_plan_facts(a, w, act, dact, aux_out, out_group, resid_mod, drop, alpha, out_t, out32, resid, resid_t, rowsum, lnfold, resid_ln))[0]
    tile_cfg, base_cfg = launch.tile_cfg, launch.base
    d.W, d.w_kblocked = (_p(ext.kb if ext is not None else packed.kblocked()), 1) if launch.w_kblocked else (_p(wrow), 0)
    d.alpha = alpha
    d.act, d.dact = _ACT[act], _ACT[dact]
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == d.N
        d.bias = _p(bias)
    for name, t, want in (("aux_in", aux_in, a.dtype), ("aux_out", aux_out, a.dtype), ("resid_t", resid_t, a.dtype),
                          ("resid", resid, torch.float32), ("out32", out32, torch.float32)):
        if t is not None and t.dtype != want:
            raise UiaError(f"gemm {name} must be {want}, got {t.dtype}")
    for name, t in (("aux_in", aux_in), ("aux_out", aux_out), ("resid_t", resid_t), ("out32", out32)):
        if t is not None and (t.dim() != 2 or t.shape[1] < d.N or (t.shape[0] < d.M and out_group == 0)):
            raise UiaError(f"gemm {name} is {tuple(t.shape)}: too small for the [{d.M}, {d.N}] result")
    if resid is not None and resid_mod == 0 and out_group == 0 and (resid.dim() != 2 or resid.shape[1] < d.N or resid.shape[0] < d.M):
        raise UiaError(f"gemm resid is {tuple(resid.shape)}: too small for the [{d.M}, {d.N}] result")
    if aux_in is not None:
        d.aux_in, d.ldaux_in = _p(aux_in), _rowmajor(aux_in, "aux_in")
    if aux_out is not None:
        d.aux_out, d.ldaux_out = _p(aux_out), _rowmajor(aux_out, "aux_out")
    if resid is not None:
        d.resid, d.ldr = _p(resid), _rowmajor(resid, "resid")
    d.resid_mod, d.resid_row_off, d.out_group = resid_mod, resid_row_off, out_group
    if resid_ln is not None:
        st, lw, lb = resid_ln[:3]
        if len(resid_ln) > 3:
            d.resid_ln_dim, d.resid_ln_eps = int(resid_ln[3]), float(resid_ln[4])
        if (resid is None and resid3 is None) or resid_mod or out_group:
            raise UiaError("gemm resid_ln needs a plain fp32 resid or a three-byte resid3 (no row remapping)")
        want_st = torch.int64 if len(resid_ln) > 3 else torch.float32       # row sums (fixed point) or (mean, rstd)
        if not (st.dtype == want_st and lw.dtype == lb.dtype == torch.float32 and st.is_contiguous() and st.numel() >= 2 * d.M and lw.numel() >= d.N and lb.numel() >= d.N):
            raise UiaError(f"gemm resid_ln: stats {tuple(st.shape)} / weight {tuple(lw.shape)} / bias {tuple(lb.shape)} do not cover [{d.M}, {d.N}]")
        d.resid_ln_stats, d.resid_ln_w, d.resid_ln_b = _p(st), _p(lw), _p(lb)
    if rowsum is not None:
        if not (rowsum.dtype == torch.int64 and rowsum.is_contiguous() and rowsum.numel() >= 2 * d.M) or out_group:
            raise UiaError(f"gemm rowsum must be a contiguous int64 [{d.M}, 2] tensor (no row remapping), got {tuple(rowsum.shape)} {rowsum.dtype}")
        d.rowsum_out = _p(rowsum)
    if lnfold is not None:
        sm, cs, dim, eps = lnfold
        if not (sm.dtype == torch.int64 and cs.dtype == torch.float32 and sm.is_contiguous() and cs.is_contiguous() and sm.numel() >= 2 * d.M and cs.numel() >= d.N) or alpha != 1.0:
            raise UiaError(f"gemm lnfold: sums {tuple(sm.shape)} {sm.dtype} / colsum {tuple(cs.shape)} do not cover [{d.M}, {d.N}] (int64 row sums, fp32 colsum, contiguous, alpha == 1)")
        d.lnfold_sums, d.lnfold_colsum, d.lnfold_dim, d.lnfold_eps = _p(sm), _p(cs), int(dim), float(eps)
    if (rowsum is not None or lnfold is not None) and a.is_cuda:
        d.ln_flag, d.ln_flag_limit = _p(ln_flag(a.device)), LN_FLAG_LIMIT
    if resid_t is not None:
        d.residT, d.ldrT = _p(resid_t), _rowmajor(resid_t, "resid_t")
    if resid3 is not None:
        if resid is not None or resid_t is not None:
            raise UiaError("gemm: resid3 replaces resid / resid_t")
        t, d.ldrT, d.residT_kb_rows = _plane(resid3[0], "resid3 hi plane", d.M, d.N, torch.bfloat16)
        d.residT = _p(t)
        t, d.ld_resid_lo, d.resid_lo_kb_rows = _plane(resid3[1], "resid3 low bytes", d.M, d.N, torch.int8)      # K-blocked: in 64-column blocks, int8 [N/64, rows, 64]
        d.resid_lo8 = _p(t)
    if out_lo is not None:
        if out_t is None:
            raise UiaError("gemm out_lo needs out_t (the hi plane)")
        t, d.ld_out_lo, d.out_lo_kb_rows = _plane(out_lo, "out_lo", d.M, d.N, torch.int8)
        d.out_lo8 = _p(t)
    if out_t is not None:
        if out_group and is_kb(out_t):
            raise UiaError(f"gemm out_t (K-blocked {tuple(out_t.t.shape)}) does not hold the [{d.M}, {d.N}] result of a row-remapping launch")
        t, d.ldo, d.outT_kb_rows = _plane(out_t, "out_t", d.M, d.N, a.dtype, not out_group)
        d.outT = _p(t)
    if out32 is not None:
        d.out32, d.ldo32 = _p(out32), _rowmajor(out32, "out32")
    if GEMM_PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib().uia_gemm(_stream(), _code(a.dtype), C.byref(d), tile_cfg), "uia_gemm")
        e1.record()
        # algorithmic HBM bytes of this launch: every operand and result once
        nbytes = esz * (d.M * d.K + d.N * d.K) + d.M * d.N * (esz * sum(t is not None for t in (aux_in, aux_out, resid_t, out_t))
                                                             + 4 * sum(t is not None for t in (resid, out32)) + 3 * (resid3 is not None) + 1 * (out_lo is not None))
        mask = epi_mask_of(d)
        if not (tile_cfg & 255) and base_cfg != 23:
            base_cfg = auto_tile_cfg(d.M, d.N, d.K, esz, mask)
        GEMM_PROFILE.append((e0, e1, d.M, d.N, d.K, a.dtype, base_cfg, nbytes, mask))
        return
    if _TRACE_GENERIC is not None:             # UIA_TRACE_GENERIC=1: which large launches land on the run-time epilogue (a mask worth a compile-time instantiation?)
        mask = epi_mask_of(d)
        if mask not in _SPECIALISED and d.M > 2048:
            _TRACE_GENERIC[(mask, d.M, d.N, d.K, base_cfg)] = _TRACE_GENERIC.get((mask, d.M, d.N, d.K, base_cfg), 0) + 1
    check(lib().uia_gemm(_stream(), _code(a.dtype), C.byref(d), tile_cfg), "uia_gemm")


def three_byte_to_float(hi, lo):
    """The fp32 values of a three-byte tensor: hi = bf16 plane (row-major or KBlocked), lo = int8 plane; float bits = (hi_bits << 16) + (lo << 8)."""
    h = hi.t.permute(1, 0, 2).reshape(hi.rows, hi.cols) if is_kb(hi) else hi
    lo = lo.t.permute(1, 0, 2).reshape(lo.rows, lo.cols) if is_kb(lo) else lo
    h = h[:lo.shape[0], :lo.shape[1]]
    bits = (h.contiguous().view(torch.int16).to(torch.int32) << 16) + (lo.to(torch.int32) << 8)
    return bits.view(torch.float32)


def float_to_three_byte(x):
    """(hi bf16, lo int8) of fp32 `x`, the arithmetic of the GEMM epilogue: hi = round-to-nearest bf16, lo = ((bits + 0x80) >> 8) - (hi_bits << 8) clamped to ±127."""
    hi = x.bfloat16()
    xb = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    hb = hi.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
    d = ((xb + 0x80) >> 8) - (hb << 8)
    return hi, d.clamp(-127, 127).to(torch.int8)


def wgrad(a, b, dw, dbias=None, alpha=1.0, drop=None):
    """dw[I,J] += alpha * a.T @ b   (a [M,I], b [M,J]); dbias[I] += a.sum(0).  dw/dbias fp32, pre-zeroed or accumulating.
    dw may be SMALLER than [I, J] (a LoRA factor's own [out, r] / [r, in] gradient under 64-padded operands): only its extent is accumulated."""
    lda, ldb = _rowmajor(a, "a"), _rowmajor(b, "b")
    assert a.dtype == b.dtype and a.shape[0] == b.shape[0] and dw.dtype == torch.float32 and dw.is_contiguous() and dw.dim() == 2
    I, J = a.shape[1], b.shape[1]
    if drop is not None:
        # drop = (p, seed): b holds the UN-dropped rows of a [M, J] tensor (row stride ldb); the mask the forward drew for it is regenerated in the staging
        p, seed = drop
        if dbias is not None or a.dtype != torch.bfloat16 or ldb != J:
            raise UiaError("wgrad(drop=...): bf16, no bias, and b must be the whole dropped tensor (contiguous rows)")
        check(lib().uia_wgrad_drop(_stream(), _code(a.dtype), a.shape[0], I, J, _p(a), lda, _p(b), ldb, alpha, _p(dw), dw.shape[1], dw.shape[0], dw.shape[1],
                                   float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, J, 0), "uia_wgrad_drop")
        return
    if tuple(dw.shape) == (I, J):
        check(lib().uia_wgrad(_stream(), _code(a.dtype), a.shape[0], I, J, _p(a), lda, _p(b), ldb, alpha, _p(dw), _p(dbias)), "uia_wgrad")
        return
    assert dw.shape[0] <= I and dw.shape[1] <= J and (dbias is None or dbias.numel() >= dw.shape[0])
    check(lib().uia_wgrad_ex(_stream(), _code(a.dtype), a.shape[0], I, J, _p(a), lda, _p(b), ldb, alpha, _p(dw), dw.shape[1], dw.shape[0], dw.shape[1],
                             _p(dbias)), "uia_wgrad_ex")


LORA_WGRAD_GROUP = True   # LoRA attention block: the dB (and the dA) weight gradients of q, k and v in ONE launch each (uia_wgrad_group) instead of three; A/B: bench.py --no-lora-wgrad-group


def wgrad_group(a_list, b_list, dw_list, dbias_list=None, alpha=1.0, drop=None):
    """dw_list[g][I', J'] += alpha * a_list[g].T @ b_list[g] for up to four problems of one shape in one launch (uia_wgrad_group); dbias_list[g] += a_list[g].sum(0) where given.
    drop = (p, seeds): b_list[g] holds UN-dropped rows of a contiguous [M, J] tensor and problem g's mask is regenerated from seeds[g] (as wgrad(drop=...) does)."""
    n = len(a_list)
    a0, b0, w0 = a_list[0], b_list[0], dw_list[0]
    if not (1 <= n <= 4 and len(b_list) == n and len(dw_list) == n and a0.dtype == torch.bfloat16):
        raise UiaError("wgrad_group: 1..4 bf16 problems")
    lda, ldb = _rowmajor(a0, "a"), _rowmajor(b0, "b")
    M, I, J = a0.shape[0], a0.shape[1], b0.shape[1]
    d = WgradGroupDesc()
    d.n, d.M, d.I, d.J, d.lda, d.ldb, d.ldw = n, M, I, J, lda, ldb, w0.shape[1]
    d.i_valid, d.j_valid, d.alpha = w0.shape[0], w0.shape[1], alpha
    for g in range(n):
        a, b, w = a_list[g], b_list[g], dw_list[g]
        if (a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or tuple(a.shape) != (M, I) or tuple(b.shape) != (M, J) or _rowmajor(a, "a") != lda or _rowmajor(b, "b") != ldb
                or w.dtype != torch.float32 or not w.is_contiguous() or w.shape != w0.shape or w.shape[0] > I or w.shape[1] > J):
            raise UiaError(f"wgrad_group: problem {g} does not have the shape / strides / dtypes of problem 0")
        d.A[g], d.B[g], d.dW[g] = a.data_ptr(), b.data_ptr(), w.data_ptr()
        db = dbias_list[g] if dbias_list is not None else None
        if db is not None:
            assert db.dtype == torch.float32 and db.numel() >= w.shape[0]
            d.dbias_A[g] = db.data_ptr()
    if drop is not None:
        p_, seeds = drop
        if ldb != J or (dbias_list is not None and any(x is not None for x in dbias_list)):
            raise UiaError("wgrad_group(drop=...): no bias, and each b must be the whole dropped tensor (contiguous rows)")
        d.drop_p, d.drop_ld, d.drop_col0 = float(p_), J, 0
        for g in range(n):
            d.drop_seed[g] = int(seeds[g]) & 0xFFFFFFFFFFFFFFFF
    check(lib().uia_wgrad_group(_stream(), _code(a0.dtype), C.byref(d)), "uia_wgrad_group")


def _attn_desc(q, k, v, out, lse, B, H, L, mask, keylen, scale, dh=None):
    d = AttnDesc()
    for t in (q, k, v):
        if t.stride(-1) != 1 or t.dtype != q.dtype:
            raise UiaError("attention operands must be unit-stride in the last dim and share a dtype")
    # the head dimension is what the operand views say it is: q holds H * dh columns (round 5: callers that left the old default of 64 with a 64-wide, two-head
    # tower — the reference's own toy geometry, tests/golden/openai_clip_base.npz — had head 1 read and WRITE 64 columns past its rows)
    width = q.shape[-1]
    if width % H != 0 or (dh is not None and dh * H != width) or k.shape[-1] != width or v.shape[-1] != width:
        raise UiaError(f"attention: q / k / v are {q.shape[-1]} / {k.shape[-1]} / {v.shape[-1]} columns wide for {H} heads" + (f" of dim {dh}" if dh is not None else ""))
    dh = width // H
    if dh not in (16, 32, 64):
        raise UiaError(f"attention: head dim {dh} unsupported (16, 32 or 64): {width} columns over {H} heads")
    if not is_kb(out) and out.shape[-1] != width:
        raise UiaError(f"attention: out is {out.shape[-1]} columns wide, q / k / v {width}")
    d.q, d.k, d.v, d.ld_qkv = _p(q), _p(k), _p(v), q.stride(-2)
    assert k.stride(-2) == q.stride(-2) == v.stride(-2)
    if is_kb(out):                                     # K-blocked [B*L, H*dh] output (bf16, dh = 64): A operand of the output projection
        rows, cols, d.out_kb_rows = _kb_dims(out, "attention out")
        if rows < B * L or cols != H * dh or dh != 64 or q.dtype != torch.bfloat16:
            raise UiaError(f"attention out (K-blocked {tuple(out.t.shape)}) must hold [{B * L}, {H * dh}] bf16 with head dim 64")
        d.out, d.ldo = _p(out.t), cols
    else:
        d.out, d.ldo = _p(out), out.stride(-2)
    d.lse = _p(lse)
    d.keylen = _p(keylen)
    d.B, d.H, d.L, d.dh = B, H, L, dh
    d.mask_kind = {"none": 0, None: 0, "causal": 1, "keypad": 2}[mask]
    d.scale = scale if scale is not None else dh ** -0.5
    return d


def attn_fwd(q, k, v, out, B, H, L, lse=None, mask=None, keylen=None, scale=None, dh=None, cu_seqlens=None):
    """q,k,v: views whose element (b,l,h,d) is at base[(b*L+l)*ld + h*dh + d] (e.g. slices of the fused qkv).
    cu_seqlens (int32 [B+1], forward only): packed sequences — sequence b is rows cu[b]..cu[b+1]-1, L = the longest one."""
    d = _attn_desc(q, k, v, out, lse, B, H, L, mask, keylen, scale, dh)
    if cu_seqlens is not None:
        assert cu_seqlens.dtype == torch.int32 and cu_seqlens.is_contiguous() and cu_seqlens.numel() == B + 1
        d.cu_seqlens = _p(cu_seqlens)
    check(lib().uia_attn_fwd(_stream(), _code(q.dtype), C.byref(d)), "uia_attn_fwd")


def attn_fwd_long(q, k, v, out, B, H, L, lse=None, scale=None):
    """uia_attn_fwd_long: softmax(q kᵀ·scale) v at any L (online softmax over 64-key blocks), head dim 64, no mask, row-major out.
    Operand layout as attn_fwd: element (b, l, h, d) of q / k / v / out at row b*L + l, column h*64 + d (slices of the fused qkv are fine)."""
    if is_kb(out):
        raise UiaError("attn_fwd_long: the output must be a row-major tensor, not K-blocked")
    d = _attn_desc(q, k, v, out, lse, B, H, L, None, None, scale)
    if d.dh != 64:
        raise UiaError(f"attn_fwd_long: head dim {d.dh}, only 64 is supported")
    check(lib().uia_attn_fwd_long(_stream(), _code(q.dtype), C.byref(d)), "uia_attn_fwd_long")


ATTN_BWD_CFG = 0     # uia_attn_bwd_cfg's kernel configuration (0 = the library's choice); tools and tests switch it for A/B runs


def attn_bwd(q, k, v, out, dout, lse, dq, dk, dv, B, H, L, mask=None, keylen=None, scale=None, dh=None, cfg=None):
    d = _attn_desc(q, k, v, out, lse, B, H, L, mask, keylen, scale, dh)
    dh = d.dh
    d.dout, d.lddo = _p(dout), dout.stride(-2)
    if is_kb(dq):                                      # the fused [B*L, 3*H*dh] gradient, K-blocked (dk, dv are then None): A operand of the QKV dgrad
        rows, cols, d.dqkv_kb_rows = _kb_dims(dq, "attention dqkv")
        if rows < B * L or cols != 3 * H * dh or dh != 64 or q.dtype != torch.bfloat16 or dk is not None or dv is not None:
            raise UiaError(f"attention dqkv (K-blocked {tuple(dq.t.shape)}) must hold [{B * L}, {3 * H * dh}] bf16 with head dim 64, dk = dv = None")
        part = (H * dh // kb_group(q.dtype)) * d.dqkv_kb_rows * kb_group(q.dtype) * dq.t.element_size()      # bytes from one part's first column block to the next
        d.dq, d.dk, d.dv, d.ld_dqkv = dq.t.data_ptr(), dq.t.data_ptr() + part, dq.t.data_ptr() + 2 * part, cols
    else:
        d.dq, d.dk, d.dv, d.ld_dqkv = _p(dq), _p(dk), _p(dv), dq.stride(-2)
        assert dk.stride(-2) == dq.stride(-2) == dv.stride(-2)
    cfg = ATTN_BWD_CFG if cfg is None else cfg
    if cfg:
        check(lib().uia_attn_bwd_cfg(_stream(), _code(q.dtype), C.byref(d), int(cfg)), "uia_attn_bwd_cfg")
    else:
        check(lib().uia_attn_bwd(_stream(), _code(q.dtype), C.byref(d)), "uia_attn_bwd")


def attn_bwd_cls(q, k, v, out, dout, lse, dq, dk, dv, B, H, L, mask=None, scale=None, rows=False):
    """uia_attn_bwd_cls: attention backward for a gradient that is zero outside token 0 of every sequence.  dout [B, H*64] holds the CLS rows only;
    q / k / v / out / lse / dq / dk / dv as attn_bwd (dq K-blocked: the fused gradient, dk = dv = None).  Every element of dq, dk, dv is written.
    Head dim 64, no mask.  rows: out [B, H*64] and lse [B, H] are the compact tensors attn_fwd_cls left (uia_attn_bwd_cls_rows)."""
    if mask not in (None, "none"):
        raise UiaError(f"attn_bwd_cls: mask {mask!r}: the CLS-query backward takes unmasked attention only")
    d = _attn_desc(q, k, v, out, lse, B, H, L, None, None, scale)
    if d.dh != 64:
        raise UiaError(f"attn_bwd_cls: head dim {d.dh}, only 64 is supported")
    if dout.dim() != 2 or dout.shape[0] != B or dout.shape[1] != H * 64 or dout.stride(1) != 1 or dout.dtype != q.dtype:
        raise UiaError(f"attn_bwd_cls: dout must be [{B}, {H * 64}] {q.dtype} rows (one per sequence), got {tuple(dout.shape)} {dout.dtype}")
    compact = bool(rows)
    if compact and (is_kb(out) or out.dim() != 2 or out.shape[0] != B or out.stride(1) != 1 or out.dtype != q.dtype):
        raise UiaError(f"attn_bwd_cls(rows=True): out must be [{B}, {H * 64}] {q.dtype} rows (one per sequence)")
    if lse is None or lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != (B * H if compact else B * H * L):
        raise UiaError(f"attn_bwd_cls: lse must be a contiguous fp32 [{B}, {H}, {L}] tensor ([{B}, {H}] beside a compact out)")
    d.dout, d.lddo = _p(dout), dout.stride(0)
    if is_kb(dq):
        rows, cols, d.dqkv_kb_rows = _kb_dims(dq, "attention dqkv")
        if rows < B * L or cols != 3 * H * 64 or q.dtype != torch.bfloat16 or dk is not None or dv is not None:
            raise UiaError(f"attention dqkv (K-blocked {tuple(dq.t.shape)}) must hold [{B * L}, {3 * H * 64}] bf16 with head dim 64, dk = dv = None")
        part = (H * 64 // kb_group(q.dtype)) * d.dqkv_kb_rows * kb_group(q.dtype) * dq.t.element_size()
        d.dq, d.dk, d.dv, d.ld_dqkv = dq.t.data_ptr(), dq.t.data_ptr() + part, dq.t.data_ptr() + 2 * part, cols
    else:
        for name, t in (("dq", dq), ("dk", dk), ("dv", dv)):
            if t.dtype != q.dtype or t.dim() != 2 or t.shape[0] < B * L or t.shape[1] != H * 64 or t.stride(1) != 1 or t.stride(0) != dq.stride(0):
                raise UiaError(f"attn_bwd_cls: {name} must be [{B * L}, {H * 64}] {q.dtype} rows sharing one row stride, got {tuple(t.shape)} {t.dtype}")
        d.dq, d.dk, d.dv, d.ld_dqkv = _p(dq), _p(dk), _p(dv), dq.stride(0)
    if compact:
        check(lib().uia_attn_bwd_cls_rows(_stream(), _code(q.dtype), C.byref(d)), "uia_attn_bwd_cls_rows")
    else:
        check(lib().uia_attn_bwd_cls(_stream(), _code(q.dtype), C.byref(d)), "uia_attn_bwd_cls")


def attn_fwd_cls(q, k, v, out, B, H, L, lse=None, mask=None, keylen=None, scale=None):
    """uia_attn_fwd_cls: the attention output of token 0 of every sequence only.  q / k / v as attn_fwd (slices of the fused [B*L, 3*H*64] qkv);
    out [B, H*64] row-major rows, lse fp32 [B, H] or None; mask None or "keypad" with keylen int32 [B].  Head dim 64, L <= 288."""
    if mask not in (None, "none", "keypad"):
        raise UiaError(f"attn_fwd_cls: mask {mask!r}: none or key padding only")
    if is_kb(out) or out.dim() != 2 or out.shape[0] != B or out.shape[1] != H * 64 or out.stride(1) != 1 or out.dtype != q.dtype:
        raise UiaError(f"attn_fwd_cls: out must be [{B}, {H * 64}] {q.dtype} rows (one per sequence)")
    if q.shape[0] < B * L:
        raise UiaError(f"attn_fwd_cls: q / k / v hold {q.shape[0]} rows, {B} sequences of {L} need {B * L}")
    if lse is not None and (lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != B * H):
        raise UiaError(f"attn_fwd_cls: lse must be a contiguous fp32 [{B}, {H}] tensor")
    if mask == "keypad" and (keylen is None or keylen.dtype != torch.int32 or not keylen.is_contiguous() or keylen.numel() != B):
        raise UiaError(f"attn_fwd_cls: key padding needs keylen int32 [{B}]")
    d = _attn_desc(q, k, v, out, lse, B, H, L, mask, keylen if mask == "keypad" else None, scale)
    if d.dh != 64:
        raise UiaError(f"attn_fwd_cls: head dim {d.dh}, only 64 is supported")
    check(lib().uia_attn_fwd_cls(_stream(), _code(q.dtype), C.byref(d)), "uia_attn_fwd_cls")


def rows3_to_f32(hi, lo, stride_rows, dst):
    """dst[r] = fp32 value of row r * stride_rows of the three-byte tensor (hi bf16 plane, row-major or KBlocked; lo int8 [M, D] row-major) (uia_rows3_to_f32)."""
    rows, D = dst.shape
    if dst.dtype != torch.float32 or not dst.is_contiguous() or lo.dtype != torch.int8 or lo.dim() != 2 or lo.stride(1) != 1 or lo.shape[1] != D:
        raise UiaError(f"rows3_to_f32: dst fp32 contiguous [rows, D] and lo int8 [M, D] are required, got {tuple(dst.shape)} {dst.dtype} / {tuple(lo.shape)} {lo.dtype}")
    _require(rows > 0 and stride_rows > 0 and (rows - 1) * stride_rows < lo.shape[0], f"rows3_to_f32: {rows} rows {stride_rows} apart do not fit the {lo.shape[0]} rows of lo")
    if is_kb(hi):
        hrows, hcols, kb_rows = _kb_dims(hi, "rows3_to_f32 hi")
        _require(hi.dtype == torch.bfloat16 and hcols == D and (rows - 1) * stride_rows < hrows, "rows3_to_f32: the K-blocked hi plane must hold bf16 [M, D]")
        hp, ldhi = hi.t.data_ptr(), D
    else:
        _require(hi.dtype == torch.bfloat16 and hi.dim() == 2 and hi.stride(1) == 1 and hi.shape[1] == D and (rows - 1) * stride_rows < hi.shape[0],
                 "rows3_to_f32: the hi plane must hold bf16 [M, D] rows")
        hp, ldhi, kb_rows = hi.data_ptr(), hi.stride(0), 0
    check(lib().uia_rows3_to_f32(_stream(), rows, D, stride_rows, hp, ldhi, kb_rows, _p(lo), lo.stride(0), _p(dst)), "uia_rows3_to_f32")
    return dst


def layernorm_fwd(x, gamma, beta, eps, y_t=None, y32=None, rows=None, ldx=None, stats=None):
    """x fp32 [rows, D] (row stride ldx); y_t (bf16|fp32) and/or y32 compact [rows, D]; stats fp32 [rows, 2] receives (mean, rstd)."""
    D = gamma.numel()
    rows = x.numel() // D if rows is None else rows
    ldx = D if ldx is None else ldx
    dt = _code(y_t.dtype) if y_t is not None else _lib.F32
    if stats is not None:
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() >= 2 * rows
        check(lib().uia_layernorm_fwd_stats(_stream(), dt, rows, D, ldx, _p(x), _p(gamma), _p(beta), eps, _p(y_t), _p(y32), _p(stats)), "uia_layernorm_fwd_stats")
        return
    check(lib().uia_layernorm_fwd(_stream(), dt, rows, D, ldx, _p(x), _p(gamma), _p(beta), eps, _p(y_t), _p(y32)), "uia_layernorm_fwd")


POOL_SLICES = 32      # UIA_POOL_SLICES of include/uia_hip.h


def ln_mean_rows(x, gamma, beta, eps, row0, n, out=None):
    """x fp32 [B, L, D]: out[b] = mean over rows row0 .. row0+n-1 of LayerNorm(x[b, l]) (uia_ln_mean_rows; fixed summation order)."""
    if x.dim() != 3 or x.dtype != torch.float32 or x.stride(-1) != 1 or x.stride(1) != x.shape[2] or x.stride(0) != x.shape[1] * x.shape[2]:
        raise UiaError("ln_mean_rows: x must be a contiguous fp32 [B, L, D] tensor")
    B, L, D = x.shape
    if out is None:
        out = torch.empty(B, D, device=x.device, dtype=torch.float32)
    if out.dtype != torch.float32 or out.stride(-1) != 1 or out.shape[-1] != D or out.shape[0] != B:
        raise UiaError("ln_mean_rows: out must be fp32 [B, D] with unit column stride")
    ws = torch.empty(B * POOL_SLICES * D, device=x.device, dtype=torch.float32)
    check(lib().uia_ln_mean_rows(_stream(), B, L, int(row0), int(n), D, D, _p(x), _p(gamma), _p(beta), float(eps), _p(ws), _p(out), out.stride(0)),
          "uia_ln_mean_rows")
    return out


def layernorm_bwd(dy, x, gamma, eps, dres=None, dx32=None, dx_t=None, rows=None, ldx=None, dx_lo=None):
    """dx = dres + LN'(dy) on rows of x.  x and dres may be three-byte tensors, passed as (hi, lo) tuples (hi bf16 row-major — x's hi plane may be
    KBlocked — lo int8 [M, D]); dx_lo = int8 [M, D] makes the result a three-byte tensor whose hi plane is dx_t (dx32 may then be None)."""
    D = gamma.numel()
    rows = dy.numel() // D if rows is None else rows
    ldx = D if ldx is None else ldx
    if isinstance(x, tuple) or isinstance(dres, tuple) or dx_lo is not None:
        x_hi, x_lo = x if isinstance(x, tuple) else (None, None)
        r_hi, r_lo = dres if isinstance(dres, tuple) else (None, None)
        x_kb = r_kb = 0
        if is_kb(x_hi):
            kr, kc, x_kb = _kb_dims(x_hi, "layernorm_bwd x hi plane")
            if kr < rows or kc != D:
                raise UiaError(f"layernorm_bwd: K-blocked x hi plane {tuple(x_hi.t.shape)} does not hold [{rows}, {D}]")
            x_hi = x_hi.t
        if is_kb(r_hi):
            kr, kc, r_kb = _kb_dims(r_hi, "layernorm_bwd dres hi plane")
            if kr < rows or kc != D:
                raise UiaError(f"layernorm_bwd: K-blocked dres hi plane {tuple(r_hi.t.shape)} does not hold [{rows}, {D}]")
            r_hi = r_hi.t
        for name, t, dt_ in (("x hi", x_hi, torch.bfloat16), ("x lo", x_lo, torch.int8), ("dres hi", r_hi, torch.bfloat16), ("dres lo", r_lo, torch.int8), ("dx_lo", dx_lo, torch.int8)):
            if t is not None and (t.dtype != dt_ or not t.is_contiguous() or t.numel() < rows * D):
                raise UiaError(f"layernorm_bwd: {name} plane must be a contiguous {dt_} tensor of at least [{rows}, {D}], got {tuple(t.shape)} {t.dtype}")
        check(lib().uia_layernorm_bwd3(_stream(), _code(dy.dtype), rows, D, ldx, _p(dy), None if isinstance(x, tuple) else _p(x), _p(x_hi), _p(x_lo), x_kb, _p(gamma), eps,
                                       None if isinstance(dres, tuple) else _p(dres), _p(r_hi), _p(r_lo), r_kb, _p(dx32), _p(dx_t), _p(dx_lo)), "uia_layernorm_bwd3")
        return
    check(lib().uia_layernorm_bwd(_stream(), _code(dy.dtype), rows, D, ldx, _p(dy), _p(x), _p(gamma), eps, _p(dres), _p(dx32), _p(dx_t)), "uia_layernorm_bwd")


def layernorm_bwd_periodic(dy, x, gamma, eps, dres_rows, period, dx32=None, dx_t=None, dx_lo=None):
    """layernorm_bwd whose residual gradient exists on rows r % period == 0 only: dres_rows fp32 [ceil(M / period), D] compact (uia_layernorm_bwd_periodic).
    bf16: the result is three-byte (dx_t, dx_lo), x fp32 or a (hi, lo) tuple; fp32: dx32 and / or dx_t, x fp32.  Bit-identical to layernorm_bwd on the zero-padded rows."""
    D = gamma.numel()
    M = dy.numel() // D
    nrows = (M + period - 1) // period
    _dense(dres_rows, "layernorm_bwd_periodic: dres_rows", _F32, nrows * D, align=16)
    x_hi, x_lo = x if isinstance(x, tuple) else (None, None)
    x_kb = 0
    if is_kb(x_hi):
        kr, kc, x_kb = _kb_dims(x_hi, "layernorm_bwd_periodic x hi plane")
        if kr < M or kc != D:
            raise UiaError(f"layernorm_bwd_periodic: K-blocked x hi plane {tuple(x_hi.t.shape)} does not hold [{M}, {D}]")
        x_hi = x_hi.t
    for name, t, dt_ in (("dy", dy, dy.dtype), ("x", None if isinstance(x, tuple) else x, torch.float32), ("x hi", x_hi, torch.bfloat16), ("x lo", x_lo, torch.int8),
                         ("dx32", dx32, torch.float32), ("dx_t", dx_t, dy.dtype), ("dx_lo", dx_lo, torch.int8)):
        if t is not None and (t.dtype != dt_ or not t.is_contiguous() or t.numel() < M * D):
            raise UiaError(f"layernorm_bwd_periodic: {name} must be a contiguous {dt_} tensor of at least [{M}, {D}], got {tuple(t.shape)} {t.dtype}")
    check(lib().uia_layernorm_bwd_periodic(_stream(), _code(dy.dtype), M, D, _p(dy), None if isinstance(x, tuple) else _p(x), _p(x_hi), _p(x_lo), x_kb, _p(gamma), eps,
                                           _p(dres_rows), int(period), _p(dx32), _p(dx_t), _p(dx_lo)), "uia_layernorm_bwd_periodic")


def cast(src, dst, scale=1.0):
    _dense(src, "cast: src", _F32, align=16)
    _dense(dst, "cast: dst", _FT, src.numel(), align="v4")
    check(lib().uia_cast(_stream(), _code(dst.dtype), src.numel(), _p(src), _p(dst), scale), "uia_cast")


def transpose_cast(src, dst):
    _dense(src, "transpose_cast: src", _F32)
    _dense(dst, "transpose_cast: dst", _FT)
    _require(src.dim() == 2 and tuple(dst.shape) == (src.shape[1], src.shape[0]),
             f"transpose_cast: dst shape {tuple(dst.shape)} is not the transpose of src {tuple(src.shape)}")
    check(lib().uia_transpose_cast(_stream(), _code(dst.dtype), src.shape[0], src.shape[1], _p(src), _p(dst)), "uia_transpose_cast")


_PIN_RING, _PIN_SLOTS, _PIN_SLOT = {}, 512, 4096


def pack_table(entries, device):
    """Device-resident uia_pack_desc table for `entries` = [(src fp32 [R, C], row, row_kb, tr, tr_kb[, (rows_pad, cols_pad, scale)])] (None = form
    not wanted).  With the optional sixth element the destinations hold rows_pad x cols_pad elements (zero padding kept by the caller: the
    launch writes only the source's elements).  Returns (table tensor, n, max_elems); keep the tensors of `entries` alive as long as the table is used."""
    arr = (PackDesc * len(entries))()
    max_elems = 0
    for d, ent in zip(arr, entries):
        src, row, row_kb, tr, tr_kb = ent[:5]
        assert src.dtype == torch.float32 and src.dim() == 2 and src.is_contiguous()
        R, Cc = src.shape
        RP, CP, scale = ent[5] if len(ent) > 5 and ent[5] is not None else (R, Cc, 1.0)
        assert RP >= R and CP >= Cc
        d.src, d.rows, d.cols, d.rows_pad, d.cols_pad, d.scale = _p(src), R, Cc, RP, CP, float(scale)
        for name, t in (("row", row), ("row_kb", row_kb), ("tr", tr), ("tr_kb", tr_kb)):
            if isinstance(t, RawDest):
                assert t.view.device == src.device
                setattr(d, name, t.view.data_ptr())
            elif t is not None:
                assert t.is_contiguous() and t.numel() == RP * CP and t.device == src.device
                setattr(d, name, _p(t))
            if t is not None and name.endswith("_kb"):
                # a K-blocked form writes whole 64-byte groups along its K extent (cols for row_kb, rows for tr_kb): a padded extent that is
                # not a multiple of the group would put the last group past the destination
                g = 64 // (t.view.element_size() if isinstance(t, RawDest) else t.element_size())
                k, kp = (Cc, CP) if name == "row_kb" else (R, RP)
                if -(-k // g) * g > kp:
                    raise UiaError(f"pack_table: {name} needs its K extent {kp} >= {k} rounded up to {g}")
        max_elems = max(max_elems, R * Cc)
    nbytes = C.sizeof(arr)
    dev = torch.device(device)
    if dev.type == "cuda" and nbytes <= _PIN_SLOT:
        # through a ring of PINNED host slots and an asynchronous copy: a pageable host-to-device copy waits for the stream, and a step that builds derived weights
        # (CLIPSeg's decoder: concatenated q | k | v, conv kernels as GEMM weights — new tensors every step) paid that wait six times (1.4 ms of a host-bound 10 ms step).
        # 512 slots: the host cannot run 512 pack launches ahead of the device.
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        ring = _PIN_RING.get(key)
        if ring is None:
            ring = _PIN_RING[key] = [torch.empty(_PIN_SLOTS, _PIN_SLOT, dtype=torch.uint8).pin_memory(), 0, [None] * _PIN_SLOTS]
        i = ring[1]
        slot = ring[0][i]
        ring[1] = (i + 1) % _PIN_SLOTS
        if ring[2][i] is not None:
            ring[2][i].synchronize()        # the copy that last read this slot (512 pack launches ago: long done; a wait only if the host ran THAT far ahead — ADVICE r04)
        C.memmove(slot.data_ptr(), C.addressof(arr), nbytes)
        table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        table.copy_(slot[:nbytes], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ring[2][i] = ev
        return table, len(entries), max_elems
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()
    return raw.to(device), len(entries), max_elems


def pack_weights(table, n, max_elems, dtype):
    _dense(table, "pack_weights: table", (torch.uint8,), align=8)
    _require(table.is_cuda and table.numel() >= n * C.sizeof(PackDesc), f"pack_weights: a device table of {n} descriptors is required")
    check(lib().uia_pack_weights(_stream(), _code(dtype), n, _p(table), max_elems), "uia_pack_weights")


def im2col(img, out, patch):
    """out [B*gh*gw, ld]: ld == C*patch^2 with patch % 4 == 0 takes the vectorised kernel, anything else the padded one
    (columns beyond C*patch^2 are zero-filled, e.g. ViT-L/14: 588 -> 640 for the GEMM's K granule)."""
    _require(img.dim() == 4 and out.dim() == 2, "im2col: img [B, C, H, W] and out [rows, ld] are required")
    B, Cc, H, W = img.shape
    _require(H % patch == 0 and W % patch == 0, f"im2col: {H}x{W} image is not a whole number of {patch}-pixel patches")
    _dense(img, "im2col: img", _F32, align=16)
    _dense(out, "im2col: out", _FT)
    _require(out.shape[0] == B * (H // patch) * (W // patch) and out.shape[1] >= Cc * patch * patch,
             f"im2col: out shape {tuple(out.shape)}, expected [{B * (H // patch) * (W // patch)}, >= {Cc * patch * patch}]")
    if patch % 4 == 0 and out.shape[1] == Cc * patch * patch and W % 4 == 0:
        check(lib().uia_im2col(_stream(), _code(out.dtype), B, Cc, H, W, patch, _p(img), _p(out)), "uia_im2col")
    else:
        check(lib().uia_im2col_padded(_stream(), _code(out.dtype), B, Cc, H, W, patch, _p(img), _p(out), out.shape[1]), "uia_im2col_padded")


def fill_cls(x, cls, pos0):
    _require(x.dim() == 3, "fill_cls: x [B, N, D] is required")
    B, N, D = x.shape
    _dense(x, "fill_cls: x", _F32)
    _dense(cls, "fill_cls: cls", _F32, D)
    if pos0 is not None:
        _dense(pos0, "fill_cls: pos0", _F32, D)
    check(lib().uia_fill_cls(_stream(), B, N, D, _p(cls), _p(pos0), _p(x)), "uia_fill_cls")


def _embed_tables(what, table, pos, type0, out, rows):
    _require(table.dim() == 2 and pos.dim() == 2 and pos.shape[1] == table.shape[1] and table.shape[1] % 4 == 0,
             f"{what}: table [V, D] and pos [P, D] with D % 4 == 0 are required, got {tuple(table.shape)} and {tuple(pos.shape)}")
    D = table.shape[1]
    _dense(table, f"{what}: table", _F32, align=16)
    _dense(pos, f"{what}: pos", _F32, align=16)
    if type0 is not None:
        _dense(type0, f"{what}: type0", _F32, D, align=16)
    _dense(out, f"{what}: out", _F32, rows * D, align=16)


def embed(ids, table, pos, type0, out):
    rows, L = ids.numel(), ids.shape[-1]
    _dense(ids, "embed: ids", (torch.int64,))
    _embed_tables("embed", table, pos, type0, out, rows)
    check(lib().uia_embed(_stream(), rows, L, table.shape[1], table.shape[0], pos.shape[0], _p(ids), _p(table), _p(pos), _p(type0), _p(out)), "uia_embed")


def embed_packed(ids, pos_idx, table, pos, type0, out):
    """out[r] = table[ids[r]] + pos[pos_idx[r]] + type0 for the packed (valid) tokens r."""
    _dense(ids, "embed_packed: ids", (torch.int64,))
    _dense(pos_idx, "embed_packed: pos_idx", (torch.int64,), ids.numel())
    _embed_tables("embed_packed", table, pos, type0, out, ids.numel())
    check(lib().uia_embed_packed(_stream(), ids.numel(), out.shape[1], table.shape[0], pos.shape[0], _p(ids), _p(pos_idx), _p(table), _p(pos), _p(type0), _p(out)),
          "uia_embed_packed")


def embed_bwd(ids, dx, dtable, pad_id=-1):
    """dtable[ids[r]] += dx[r] for every row r with ids[r] != pad_id (dtable fp32, caller-zeroed or accumulating)."""
    _dense(ids, "embed_bwd: ids", (torch.int64,))
    _require(dx.dim() >= 1 and dtable.dim() == 2 and dx.shape[-1] == dtable.shape[1], "embed_bwd: dx [.., D] and dtable [V, D] are required")
    _dense(dx, "embed_bwd: dx", _F32, ids.numel() * dtable.shape[1])
    _dense(dtable, "embed_bwd: dtable", _F32)
    check(lib().uia_embed_bwd(_stream(), ids.numel(), dx.shape[-1], dtable.shape[0], _p(ids), _p(dx), _p(dtable), pad_id), "uia_embed_bwd")


def gather_rows(src, idx, dst):
    """dst[i] = src[idx[i]]; idx must lie in [0, src rows): the kernel reads it unchecked."""
    _dense(idx, "gather_rows: idx", (torch.int64,))
    _require(src.dim() >= 1 and src.shape[-1] % 4 == 0, "gather_rows: src [.., D] with D % 4 == 0 is required")
    _dense(src, "gather_rows: src", _F32, align=16)
    _dense(dst, "gather_rows: dst", _F32, idx.numel() * src.shape[-1], align=16)
    check(lib().uia_gather_rows(_stream(), idx.numel(), src.shape[-1], _p(src), _p(idx), _p(dst)), "uia_gather_rows")


def copy_rows(src, stride_rows, dst):
    """dst[r] = src[r * stride_rows] for the rows of dst: every stride_rows-th row of a contiguous [M, W] tensor of any dtype (uia_copy_rows;
    the CLS rows of a saved activation: stride_rows = tokens per image).  Rows are whole 16-byte units."""
    if src.dim() != 2 or dst.dim() != 2 or not src.is_contiguous() or not dst.is_contiguous() or src.dtype != dst.dtype or src.shape[1] != dst.shape[1]:
        raise UiaError(f"copy_rows: contiguous 2-D tensors of one dtype and width are required, got {tuple(src.shape)} {src.dtype} -> {tuple(dst.shape)} {dst.dtype}")
    rows, row_bytes = dst.shape[0], src.shape[1] * src.element_size()
    _require(rows > 0 and stride_rows > 0 and (rows - 1) * stride_rows < src.shape[0], f"copy_rows: {rows} rows {stride_rows} apart do not fit the {src.shape[0]} rows of src")
    _require(row_bytes % 16 == 0 and src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0, "copy_rows: rows must be whole, aligned 16-byte units")
    check(lib().uia_copy_rows(_stream(), rows, row_bytes, _p(src), row_bytes * stride_rows, _p(dst)), "uia_copy_rows")
    return dst


# ------------------------------------------------------------------------------------------- Mona
_SPATIAL_KEYS = ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "conv3_w", "conv3_b", "proj_w", "proj_b", "freq", "ne1_w", "ne1_b", "ne3_w", "ne3_b")


def mona_pre_fwd(x, norm_w, norm_b, gamma, gammax, u, eps=1e-5, proj1=None):
    """proj1 = (w1 [64, D] T row-major, b1 fp32 [64] or None, t [M, 64] T): project1 runs inside the launch (uia_mona_pre_fwd_t: bf16, D = 768)."""
    D = gamma.numel()
    if proj1 is not None:
        w1, b1, t = proj1
        M = x.numel() // D
        if u.dtype != torch.bfloat16 or w1.dtype != u.dtype or t.dtype != u.dtype or tuple(w1.shape) != (64, D) or tuple(t.shape) != (M, 64):
            raise UiaError(f"mona_pre_fwd proj1: w1 {tuple(w1.shape)} / t {tuple(t.shape)} must be bf16 [64, {D}] / [{M}, 64]")
        check(lib().uia_mona_pre_fwd_t(_stream(), _code(u.dtype), M, D, _p(x), _p(norm_w), _p(norm_b), _p(gamma), _p(gammax), eps, _p(u), _p(w1), _rowmajor(w1, "w1"),
                                       _p(b1), _p(t), _rowmajor(t, "t")), "uia_mona_pre_fwd_t")
        return
    check(lib().uia_mona_pre_fwd(_stream(), _code(u.dtype), x.numel() // D, D, _p(x), _p(norm_w), _p(norm_b), _p(gamma), _p(gammax), eps, _p(u)), "uia_mona_pre_fwd")


def mona_pre_bwd_du_ok(M, D, bott, dt):
    """Shapes uia_mona_pre_bwd_du takes: bf16, bottleneck 64, D a multiple of 64 up to 768 (the row kernel's three-float4-per-lane instantiation)."""
    return MONA_PRE_BWD_DU and dt == torch.bfloat16 and bott == 64 and D % 64 == 0 and 512 < D <= 768


def mona_pre_bwd(du, x, dy, norm_w, norm_b, gamma, gammax, dx32, dx_t, g_gamma, g_gammax, g_norm_w, g_norm_b, eps=1e-5, dt_w1t=None, dx_lo=None):
    """dt_w1t = (dt [M, 64], W1ᵀ [D, 64]) instead of du: project1's data gradient du = dt·W1 is computed inside the launch (uia_mona_pre_bwd_du).
    Three-byte residual gradients (uia_mona_pre_bwd_du3, with dt_w1t only): dy = (hi bf16 [M, D] row-major, lo int8 [M, D]) and dx_lo = int8 [M, D] — the result
    is then (dx_t, dx_lo) and dx32 must be None."""
    D = gamma.numel()
    M = x.numel() // D
    ws = torch.empty(lib().uia_mona_pre_bwd_workspace_bytes(M, D) // 4, device=x.device, dtype=torch.float32)
    kb_rows = 0
    if is_kb(dx_t):                                    # K-blocked T copy of dx (read by a ring GEMM only)
        rows, cols, kb_rows = _kb_dims(dx_t, "mona_pre_bwd dx_t")
        if rows != M or cols != D:
            raise UiaError(f"mona_pre_bwd dx_t (K-blocked {tuple(dx_t.t.shape)}) does not hold [{M}, {D}]")
        dx_t = dx_t.t
    if dt_w1t is not None:
        dtt, w1t = dt_w1t
        if dtt.dtype != torch.bfloat16 or w1t.dtype != torch.bfloat16 or tuple(dtt.shape) != (M, 64) or tuple(w1t.shape) != (D, 64):
            raise UiaError(f"mona_pre_bwd: dt {tuple(dtt.shape)} {dtt.dtype} / W1ᵀ {tuple(w1t.shape)} {w1t.dtype} must be bf16 [{M}, 64] / [{D}, 64]")
        if isinstance(dy, tuple) or dx_lo is not None:
            if not (isinstance(dy, tuple) and dx_lo is not None and dx32 is None and dx_t is not None):
                raise UiaError("mona_pre_bwd: three-byte residual gradients need dy = (hi, lo), dx_lo and dx_t, and no dx32")
            hi, lo = dy
            for name, t_, dt_ in (("dy hi", hi, torch.bfloat16), ("dy lo", lo, torch.int8), ("dx_lo", dx_lo, torch.int8), ("dx_t", dx_t, torch.bfloat16)):
                if t_.dtype != dt_ or not t_.is_contiguous() or t_.numel() < M * D:
                    raise UiaError(f"mona_pre_bwd: {name} plane must be a contiguous {dt_} tensor of at least [{M}, {D}], got {tuple(t_.shape)} {t_.dtype}")
            check(lib().uia_mona_pre_bwd_du3(_stream(), _code(dtt.dtype), M, D, _p(dtt), _rowmajor(dtt, "dt"), _p(w1t), _rowmajor(w1t, "w1t"), _p(x), _p(hi), _p(lo), _p(norm_w),
                                             _p(norm_b), _p(gamma), _p(gammax), eps, _p(dx_t), _p(dx_lo), _p(g_gamma), _p(g_gammax), _p(g_norm_w), _p(g_norm_b), _p(ws),
                                             kb_rows), "uia_mona_pre_bwd_du3")
            return
        check(lib().uia_mona_pre_bwd_du(_stream(), _code(dtt.dtype), M, D, _p(dtt), _rowmajor(dtt, "dt"), _p(w1t), _rowmajor(w1t, "w1t"), _p(x), _p(dy), _p(norm_w),
                                        _p(norm_b), _p(gamma), _p(gammax), eps, _p(dx32), _p(dx_t), _p(g_gamma), _p(g_gammax), _p(g_norm_w), _p(g_norm_b), _p(ws),
                                        kb_rows), "uia_mona_pre_bwd_du")
        return
    check(lib().uia_mona_pre_bwd(_stream(), _code(du.dtype), M, D, _p(du), _p(x), _p(dy), _p(norm_w), _p(norm_b), _p(gamma), _p(gammax),
                                 eps, _p(dx32), _p(dx_t), _p(g_gamma), _p(g_gammax), _p(g_norm_w), _p(g_norm_b), _p(ws), kb_rows), "uia_mona_pre_bwd")


def _spatial_desc(variant, B, h, w, t, params, p_drop, seed, keep_mask):
    d = MonaSpatialDesc()
    d.variant = _lib.MONA_VARIANTS[variant]
    d.B, d.h, d.w, d.bott = B, h, w, t.shape[-1]
    d.t = _p(t)
    for k in _SPATIAL_KEYS:
        v = params.get(k)
        if v is not None:
            assert v.dtype == torch.float32 and v.is_contiguous()
            setattr(d, k, _p(v))
    d.p_drop, d.seed = float(p_drop), int(seed) & 0xFFFFFFFFFFFFFFFF
    if keep_mask is not None:
        assert keep_mask.dtype == torch.uint8 and keep_mask.is_contiguous()
        d.keep_mask = _p(keep_mask)
    return d


# The whole adapter forward in one launch (csrc/mona_fused.hip) where uia_mona_fused_supported says so.  Built, parity-tested and measured in
# round 3 (tools/mff_variants.sh, profiles/r03_c_mona_fused_phases.txt): 199 us per ViT-B/16 layer with the u stash the backward's weight
# gradient needs (181 without) against 179 us for the four unfused launches — its third phase IS the K = 64 projection with the fp32 residual
# (387 MB, ~100 us either way) and the first two save 16 us of the 98 they replace.  Opt-in until the backward recomputes u.
MONA_FUSED = False


def mona_fused_ok(dt, D, h, w, bott):
    return MONA_FUSED and dt == torch.bfloat16 and bool(lib().uia_mona_fused_supported(_code(dt), D, h, w, bott))


def mona_fused_fwd(variant, B, h, w, x, norm_w, norm_b, gamma, gammax, w1, b1, w2, b2, params, y32, y_t=None, rowsum=None, u_out=None, t_out=None, d_out=None,
                   p_drop=0.0, seed=0, keep_mask=None, eps=1e-5):
    """y32 = x + project2(drop(gelu(spatial(project1(LN(x)·gamma + x·gammax)))))  for B images of 1 + h·w tokens, one launch
    (include/uia_hip.h, uia_mona_fused_desc).  x fp32 [B, 1+h·w, D]; w1 [64, D] / w2 [D, 64] in the compute dtype; params as mona_spatial_fwd.
    y_t: optional T copy of y (tensor or KBlocked); rowsum: int64 [M, 2] receiving the rows' (Σ, Σ²); u_out / t_out / d_out: optional stashes."""
    D = x.shape[-1]
    q = MonaFusedDesc()
    sp = _spatial_desc(variant, B, h, w, w1.new_empty(0, w1.shape[0]) if t_out is None else t_out, params, p_drop, seed, keep_mask)
    sp.t = None
    if d_out is not None:
        sp.d = _p(d_out)
    q.sp = sp
    q.D, q.eps = D, eps
    assert x.dtype == torch.float32 and x.is_contiguous() and y32.dtype == torch.float32 and y32.is_contiguous() and y32.numel() == x.numel()
    assert tuple(w1.shape) == (sp.bott, D) and tuple(w2.shape) == (D, sp.bott) and w1.is_contiguous() and w2.is_contiguous() and w1.dtype == w2.dtype
    q.x, q.norm_w, q.norm_b, q.gamma, q.gammax = _p(x), _p(norm_w), _p(norm_b), _p(gamma), _p(gammax)
    q.w1, q.b1, q.w2, q.b2, q.y32 = _p(w1), _p(b1), _p(w2), _p(b2), _p(y32)
    M = B * (1 + h * w)
    if is_kb(y_t):
        rows, cols, plane = _kb_dims(y_t, "mona_fused y_t")
        if rows < M or cols != D:
            raise UiaError(f"mona_fused y_t (K-blocked {tuple(y_t.t.shape)}) does not hold [{M}, {D}]")
        q.yT, q.yT_kb_rows = _p(y_t.t), plane
    elif y_t is not None:
        assert y_t.dtype == w1.dtype and y_t.is_contiguous() and y_t.numel() == M * D
        q.yT = _p(y_t)
    if rowsum is not None:
        assert rowsum.dtype == torch.int64 and rowsum.is_contiguous() and rowsum.numel() >= 2 * M
        q.rowsum_out, q.ln_flag = _p(rowsum), _p(ln_flag(x.device))
    for name, t, width in (("u_out", u_out, D), ("t_out", t_out, sp.bott)):
        if t is not None:
            assert t.dtype == w1.dtype and t.is_contiguous() and t.numel() == M * width
            setattr(q, name, _p(t))
    check(lib().uia_mona_fused_fwd(_stream(), _code(w1.dtype), C.byref(q)), "uia_mona_fused_fwd")


def mona_spatial_fwd(variant, B, h, w, t, params, d_out, p_drop=0.0, seed=0, keep_mask=None):
    """params: dict with keys of _SPATIAL_KEYS (fp32, contiguous; absent ones for variants without them)."""
    d = _spatial_desc(variant, B, h, w, t, params, p_drop, seed, keep_mask)
    d.d = _p(d_out)
    check(lib().uia_mona_spatial_fwd(_stream(), _code(t.dtype), C.byref(d)), "uia_mona_spatial_fwd")


def mona_spatial_bwd(variant, B, h, w, t, params, dd, dt, grads, p_drop=0.0, seed=0, keep_mask=None):
    """grads: dict keyed like params with fp32 accumulators (caller-zeroed)."""
    d = _spatial_desc(variant, B, h, w, t, params, p_drop, seed, keep_mask)
    d.dd, d.dt = _p(dd), _p(dt)
    ws = torch.empty(lib().uia_mona_spatial_workspace_bytes(B) // 4, device=t.device, dtype=torch.float32)
    d.ws = _p(ws)
    for k in _SPATIAL_KEYS:
        v = grads.get(k)
        if v is not None:
            setattr(d, "g_" + k, _p(v))
    check(lib().uia_mona_spatial_bwd(_stream(), _code(t.dtype), C.byref(d)), "uia_mona_spatial_bwd")


def mona_cls_fwd(B, ntok, t, d, p_drop=0.0, seed=0, keep_mask=None):
    """The CLS token's share of mona_spatial_fwd (uia_mona_cls_fwd): t, d compact [B, 64]; the dropout mask (seed or keep_mask uint8 [B, ntok, 64]) is indexed
    as in the dense tensor of ntok tokens per image."""
    for name, x_ in (("t", t), ("d", d)):
        _dense(x_, f"mona_cls_fwd: {name}", (t.dtype,), B * 64, align=2)
    if keep_mask is not None:
        _dense(keep_mask, "mona_cls_fwd: keep_mask", (torch.uint8,), B * ntok * 64)
    check(lib().uia_mona_cls_fwd(_stream(), _code(t.dtype), B, ntok, _p(t), 64, _p(d), float(p_drop), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(keep_mask)), "uia_mona_cls_fwd")


def mona_cls_bwd(B, ntok, dd, t, dt, p_drop=0.0, seed=0, keep_mask=None, t_rows=False):
    """The CLS token's share of mona_spatial_bwd (uia_mona_cls_bwd): dd, dt compact [B, 64]; t the forward's [B * ntok, 64] tensor, read at rows b * ntok
    (t_rows: its B CLS rows alone, compact [B, 64], as mona_cls_fwd read them); the dropout mask (seed or keep_mask uint8 [B, ntok, 64]) is indexed as in the dense tensor.  No parameter gradients: the token bypasses the spatial operator."""
    for name, x_, n in (("dd", dd, B * 64), ("dt", dt, B * 64), ("t", t, B * 64 if t_rows else B * ntok * 64)):
        _dense(x_, f"mona_cls_bwd: {name}", (t.dtype,), n, align=2)
    if keep_mask is not None:
        _dense(keep_mask, "mona_cls_bwd: keep_mask", (torch.uint8,), B * ntok * 64)
    check(lib().uia_mona_cls_bwd(_stream(), _code(t.dtype), B, ntok, _p(dd), _p(t), 64 if t_rows else ntok * 64, _p(dt), float(p_drop), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(keep_mask)),
          "uia_mona_cls_bwd")


# ------------------------------------------------------------------------------------------- loss / optimiser / comm
def infonce(img, txt, temperature, grad_scale=1.0, want_grads=True):
    """Returns (loss[1] fp32 device tensor, dimg, dtxt).  img/txt fp32 [B,E] contiguous."""
    assert img.dtype == torch.float32 and txt.dtype == torch.float32 and img.is_contiguous() and txt.is_contiguous()
    B, E = img.shape
    nbytes = lib().uia_infonce_workspace_bytes(B, E)
    ws = torch.empty(nbytes // 4, device=img.device, dtype=torch.float32)
    loss = torch.empty(1, device=img.device, dtype=torch.float32)
    dimg = torch.empty_like(img) if want_grads else None
    dtxt = torch.empty_like(txt) if want_grads else None
    check(lib().uia_infonce_fwd_bwd(_stream(), B, E, _p(img), _p(txt), 1.0 / temperature, grad_scale, _p(loss), _p(dimg), _p(dtxt), _p(ws), nbytes), "uia_infonce_fwd_bwd")
    return loss, dimg, dtxt


def adamw_clip_step(p, g, m, v, lr, betas, eps, weight_decay, max_norm, step, grad_scale, ws2):
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()
    check(lib().uia_adamw_clip_step(_stream(), p.numel(), _p(p), _p(g), _p(m), _p(v), lr, betas[0], betas[1], eps, weight_decay, max_norm, step, grad_scale, _p(ws2)), "uia_adamw_clip_step")


def grad_accum_guarded(acc, mb, loss, stats, ctl, ok_log=None, log_index=0):
    """acc [n + 4] += mb [n] when the device loss is finite; mb zeroed; acc[n] = this micro-batch's flag (include/uia_hip.h)."""
    n = mb.numel()
    assert acc.dtype == mb.dtype == loss.dtype == stats.dtype == torch.float32 and acc.numel() >= n + 4 and ctl.dtype == torch.int32 and ctl.numel() >= 4
    assert ok_log is None or (ok_log.dtype == torch.uint8 and 0 <= log_index < ok_log.numel())
    check(lib().uia_grad_accum_guarded(_stream(), n, _p(acc), _p(mb), _p(loss), _p(stats), _p(ctl), _p(ok_log), int(log_index)), "uia_grad_accum_guarded")


def adamw_clip_step_guarded(p, acc, m, v, lr, lr_min, t_max, betas, eps, weight_decay, max_norm, grad_scale, skip_scale, ws8, ctl):
    n = p.numel()
    for t in (p, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    assert acc.dtype == torch.float32 and acc.numel() >= n + 4 and ws8.numel() >= 8 and ctl.dtype == torch.int32 and ctl.numel() >= 4
    check(lib().uia_adamw_clip_step_guarded(_stream(), n, _p(p), _p(acc), _p(m), _p(v), lr, lr_min, int(t_max), betas[0], betas[1], eps, weight_decay, max_norm,
                                            grad_scale, skip_scale, _p(ws8), _p(ctl)), "uia_adamw_clip_step_guarded")


def comm_unique_id():
    n = lib().uia_comm_unique_id_bytes()
    buf = C.create_string_buffer(n)
    check(lib().uia_comm_get_unique_id(buf, n), "uia_comm_get_unique_id")
    return bytes(buf.raw)


def comm_init(rank, world, uid):
    check(lib().uia_comm_init(rank, world, C.c_char_p(uid), len(uid)), "uia_comm_init")


def comm_world():
    return lib().uia_comm_world()


def comm_world_initialised():
    return bool(lib().uia_comm_initialised())


def allreduce_sum(buf):
    import os
    try:
        check(lib().uia_allreduce_sum(_stream(), _code(buf.dtype), _p(buf), buf.numel()), "uia_allreduce_sum")
    except UiaError as e:                                       # say WHICH rank: the others are most likely blocked inside the collective
        raise UiaError(f"rank {os.environ.get('RANK', '0')}/{os.environ.get('WORLD_SIZE', '1')}: {e}") from e


def allgather(send, recv):
    """recv [world * n] = concatenation over ranks of send [n] (same dtype, contiguous)."""
    assert send.is_contiguous() and recv.is_contiguous() and send.dtype == recv.dtype and recv.numel() == send.numel() * comm_world()
    check(lib().uia_allgather(_stream(), _code(send.dtype), _p(send), _p(recv), send.numel()), "uia_allgather")


def comm_destroy():
    check(lib().uia_comm_destroy(), "uia_comm_destroy")


def dropout(src, dst, p, seed, accumulate=False):
    assert src.dtype == dst.dtype and src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    check(lib().uia_dropout(_stream(), _code(src.dtype), src.numel(), _p(src), _p(dst), p, int(seed) & 0xFFFFFFFFFFFFFFFF, int(accumulate)), "uia_dropout")


def ln_lora_down_ok(D, r, dt):
    """Shapes uia_ln_lora_down takes: bf16, D = 768 or 1024, rank <= 16."""
    return LN_LORA_DOWN and dt == torch.bfloat16 and D in (768, 1024) and 0 < r <= 16


def ln_lora_down(x, gamma, beta, eps, h, a_rows, t_all, drop_p=0.0, seeds=()):
    """h = LayerNorm(x) (T [M, D], written) and t_all[s] = dropout_s(h) @ a_rows[s][:16].T for up to three LoRA wrappers sharing the input, in one launch.
    a_rows: T [>= 16, D] each (rank rows, zero-padded); t_all: T [n, M, 64] contiguous — columns 16..63 are written as zeros."""
    n, M, w = t_all.shape
    D = gamma.numel()
    if not (t_all.is_contiguous() and w == 64 and len(a_rows) == n and tuple(h.shape) == (M, D) and h.is_contiguous() and x.dtype == torch.float32 and x.shape[-1] == D):
        raise UiaError(f"ln_lora_down: x {tuple(x.shape)}, h {tuple(h.shape)}, t_all {tuple(t_all.shape)}")
    if drop_p > 0 and len(seeds) != n:
        raise UiaError("ln_lora_down: one dropout seed per source")
    d = LnLoraDesc()
    d.M, d.D, d.nsrc, d.eps = M, D, n, float(eps)
    d.x, d.ldx = _p(x), _rowmajor(x, "x")
    d.gamma, d.beta, d.h = _p(gamma), _p(beta), _p(h)
    lda = None
    for i, a in enumerate(a_rows):
        if a.dtype != h.dtype or a.dim() != 2 or a.shape[0] < 16 or a.shape[1] != D:
            raise UiaError(f"ln_lora_down: factor {i} is {tuple(a.shape)} {a.dtype}, expected [>= 16, {D}] {h.dtype}")
        l = _rowmajor(a, "a")
        if lda is not None and l != lda:
            raise UiaError("ln_lora_down: the factors must share one leading dimension")
        lda = l
        d.A[i] = _p(a)
    d.lda = lda
    d.T, d.t_stride = _p(t_all), M * 64
    d.drop_p = float(drop_p)
    for i in range(n if drop_p > 0 else 0):
        d.seed[i] = int(seeds[i]) & 0xFFFFFFFFFFFFFFFF
    check(lib().uia_ln_lora_down(_stream(), _code(h.dtype), C.byref(d)), "uia_ln_lora_down")


def lora_rank_update_ok(n_src, N, dt):
    """Shapes uia_lora_rank_update takes: bf16, N a multiple of 256, the sources' [N/4, 64] weight rows inside the LDS."""
    return dt == torch.bfloat16 and 1 <= n_src <= 3 and N % 256 == 0 and n_src * (N // 4) * 144 <= 160 * 1024


def lora_rank_update(q_all, ws, out, alpha, drop_p=0.0, seeds=()):
    """out += sum_i drop_i(alpha * q_all[i] @ ws[i].T) in ONE read-modify-write pass over `out` (uia_lora_rank_update, csrc/lora_rank.hip).
    q_all: T [n, M, 64] (contiguous); ws: n matrices T [N, 64] (A_i transposed, rank zero-padded to 64); out: T [M, N] row-major;
    seeds: one per source when drop_p > 0 — the masks are those uia_dropout / gemm(drop=("acc", p, seed)) draw for an [M, N] tensor."""
    n, M, r = q_all.shape
    N = out.shape[1]
    if not (q_all.is_contiguous() and r == 64 and out.shape[0] == M and len(ws) == n and lora_rank_update_ok(n, N, out.dtype) and q_all.dtype == out.dtype):
        raise UiaError(f"lora_rank_update: q_all {tuple(q_all.shape)} {q_all.dtype}, out {tuple(out.shape)} {out.dtype}, {len(ws)} weights")
    if drop_p > 0 and len(seeds) != n:
        raise UiaError("lora_rank_update: one dropout seed per source")
    d = LoraRankDesc()
    d.M, d.N, d.nsrc, d.alpha = M, N, n, float(alpha)
    d.Q, d.ldq, d.q_stride = _p(q_all), 64, M * 64
    ldw = None
    for i, w in enumerate(ws):
        if w.dtype != out.dtype or tuple(w.shape) != (N, 64):
            raise UiaError(f"lora_rank_update: weight {i} is {tuple(w.shape)} {w.dtype}, expected [{N}, 64] {out.dtype}")
        l = _rowmajor(w, "w")
        if ldw is not None and l != ldw:
            raise UiaError("lora_rank_update: the weights must share one leading dimension")
        ldw = l
        d.W[i] = _p(w)
    d.ldw = ldw
    d.out, d.ldo = _p(out), _rowmajor(out, "out")
    d.drop_p = float(drop_p)
    for i in range(n if drop_p > 0 else 0):
        d.seed[i] = int(seeds[i]) & 0xFFFFFFFFFFFFFFFF
    check(lib().uia_lora_rank_update(_stream(), _code(out.dtype), C.byref(d)), "uia_lora_rank_update")


def colsum(a, out):
    lda = _rowmajor(a, "colsum: a")
    _require(a.dtype in _FT, f"colsum: a dtype {a.dtype}, expected bf16 or fp32")
    _dense(out, "colsum: out", _F32, a.shape[1])
    check(lib().uia_colsum(_stream(), _code(a.dtype), a.shape[0], a.shape[1], _p(a), lda, _p(out)), "uia_colsum")


# ------------------------------------------------------------------------------------------- CLIPSeg decoder pieces
def layernorm_bwd_affine(dy, x, gamma, eps, dx32, g_gamma, g_beta, dres=None):
    """dx32 = LayerNorm backward of the fp32 rows x (+ dres); dγ, dβ are ADDED into g_gamma / g_beta.  dy in T (bf16 or fp32)."""
    D = _dense(gamma, "layernorm_bwd_affine: gamma", _F32, align=16).numel()
    _dense(dy, "layernorm_bwd_affine: dy", _FT, align="v4")
    _require(D > 0 and dy.numel() % D == 0, f"layernorm_bwd_affine: dy has {dy.numel()} elements, not a whole number of rows of D = {D}")
    for name, t in (("x", x), ("dx32", dx32), ("dres", dres)):
        if t is not None or name != "dres":
            _dense(t, f"layernorm_bwd_affine: {name}", _F32, dy.numel(), align=16)
    for name, t in (("g_gamma", g_gamma), ("g_beta", g_beta)):
        _dense(t, f"layernorm_bwd_affine: {name}", _F32, D, align=16)
    check(lib().uia_layernorm_bwd_affine(_stream(), _code(dy.dtype), dy.numel() // D, D, _p(dy), _p(x), _p(gamma), eps, _p(dres), _p(dx32), _p(g_gamma), _p(g_beta)),
          "uia_layernorm_bwd_affine")


def film_fwd(x, mul, add, y):
    _require(x.dim() == 3, "film_fwd: x [B, N, C] is required")
    B, N, Cc = x.shape
    _dense(x, "film_fwd: x", _F32, align=16)
    _dense(mul, "film_fwd: mul", _F32, B * Cc, align=16)
    _dense(add, "film_fwd: add", _F32, B * Cc, align=16)
    _dense(y, "film_fwd: y", _F32, x.numel(), align=16)
    check(lib().uia_film_fwd(_stream(), B, N, Cc, _p(x), _p(mul), _p(add), _p(y)), "uia_film_fwd")


def film_bwd(dy, x, mul, dx, dmul, dadd):
    _require(x.dim() == 3, "film_bwd: x [B, N, C] is required")
    B, N, Cc = x.shape
    for name, t, n in (("dy", dy, x.numel()), ("x", x, None), ("dx", dx, x.numel()), ("mul", mul, B * Cc), ("dmul", dmul, B * Cc), ("dadd", dadd, B * Cc)):
        _dense(t, f"film_bwd: {name}", _F32, n)
    check(lib().uia_film_bwd(_stream(), B, N, Cc, _p(dy), _p(x), _p(mul), _p(dx), _p(dmul), _p(dadd)), "uia_film_bwd")


def im2col3x3(x, cols, h, w, tok_off=1):
    _require(x.dim() == 3, "im2col3x3: x [B, ntok, C] is required")
    B, N, Cc = x.shape
    _require(0 <= tok_off and tok_off + h * w <= N, f"im2col3x3: tokens {tok_off} .. {tok_off + h * w} outside the {N} rows of x")
    _dense(x, "im2col3x3: x", _F32, align=16)
    _dense(cols, "im2col3x3: cols", _FT, B * h * w * 9 * Cc, align="v4")
    check(lib().uia_im2col3x3(_stream(), _code(cols.dtype), B, h, w, Cc, N, tok_off, _p(x), _p(cols)), "uia_im2col3x3")


def col2im3x3(dcols, dx, h, w, tok_off=1):
    _require(dx.dim() == 3, "col2im3x3: dx [B, ntok, C] is required")
    B, N, Cc = dx.shape
    _require(0 <= tok_off and tok_off + h * w <= N, f"col2im3x3: tokens {tok_off} .. {tok_off + h * w} outside the {N} rows of dx")
    _dense(dx, "col2im3x3: dx", _F32, align=16)
    _dense(dcols, "col2im3x3: dcols", _FT, B * h * w * 9 * Cc, align="v4")
    check(lib().uia_col2im3x3(_stream(), _code(dcols.dtype), B, h, w, Cc, N, tok_off, _p(dcols), _p(dx)), "uia_col2im3x3")


def _shuffle_rows(what, tmp, B, h, w, k1, k2):
    ld = _rowmajor(tmp, f"{what}: tmp")
    _require(tmp.dtype in _FT, f"{what}: tmp dtype {tmp.dtype}, expected bf16 or fp32")
    _require(tmp.shape[0] == B * h * w * k1 * k1 and tmp.shape[1] >= k2 * k2,
             f"{what}: tmp shape {tuple(tmp.shape)}, expected [{B * h * w * k1 * k1}, >= {k2 * k2}]")
    return ld


def unshuffle(tmp, out, B, h, w, k1, k2, bias=0.0):
    _shuffle_rows("unshuffle", tmp, B, h, w, k1, k2)
    _dense(out, "unshuffle: out", _F32, B * h * w * (k1 * k2) ** 2)
    check(lib().uia_unshuffle(_stream(), _code(tmp.dtype), B, h, w, k1, k2, _p(tmp), tmp.stride(0), bias, _p(out)), "uia_unshuffle")


def shuffle(dout, dtmp, B, h, w, k1, k2):
    """dtmp [B·h·w·k1², ld]: every column is written, the ones beyond k2² with zeros, so dtmp must be contiguous (ld = its width)."""
    _shuffle_rows("shuffle", dtmp, B, h, w, k1, k2)
    _dense(dtmp, "shuffle: dtmp", _FT)
    _dense(dout, "shuffle: dout", _F32, B * h * w * (k1 * k2) ** 2)
    check(lib().uia_shuffle(_stream(), _code(dtmp.dtype), B, h, w, k1, k2, _p(dout), _p(dtmp), dtmp.stride(0)), "uia_shuffle")


def act_bwd(dy, y, act, out):
    """out = dy · act'(y) elementwise; y is the post-activation for ReLU, the pre-activation for GELU / QuickGELU."""
    _require(act in _ACT, f"act_bwd: unknown activation {act!r}")
    _dense(dy, "act_bwd: dy", _FT)
    _dense(y, "act_bwd: y", (dy.dtype,), dy.numel())
    _dense(out, "act_bwd: out", (dy.dtype,), dy.numel())
    check(lib().uia_act_bwd(_stream(), _code(dy.dtype), dy.numel(), _p(dy), _p(y), _ACT[act], _p(out)), "uia_act_bwd")


# ------------------------------------------------------------------------------------------- FPN task heads
def upsample_bilinear(src, B, C, h, w, H, W, dst, backward=False):
    """forward: src token-major fp32 [B*h*w, ld>=C] -> dst [B,C,H,W]; backward: src = d(dst) [B,C,H,W] -> dst token-major (overwritten)."""
    tok = dst if backward else src
    _rowmajor(tok, "upsample_bilinear: token rows")
    _require(tok.dtype == torch.float32 and tok.shape[0] == B * h * w and tok.shape[1] >= C,
             f"upsample_bilinear: token rows {tuple(tok.shape)} {tok.dtype}, expected fp32 [{B * h * w}, >= {C}]")
    img = src if backward else dst
    _dense(img, "upsample_bilinear: image", _F32, B * C * H * W)
    _require(tuple(img.shape) == (B, C, H, W), f"upsample_bilinear: image shape {tuple(img.shape)}, expected {(B, C, H, W)}")
    if backward:
        check(lib().uia_upsample_bilinear_bwd(_stream(), B, C, h, w, H, W, _p(src), _p(dst), dst.stride(0)), "uia_upsample_bilinear_bwd")
    else:
        check(lib().uia_upsample_bilinear_fwd(_stream(), B, C, h, w, H, W, _p(src), src.stride(0), _p(dst)), "uia_upsample_bilinear_fwd")


def segment_mean(x, B, n, out, backward=False):
    """forward: x fp32 [B*n, C] -> out [B, C] (mean over each image's n tokens); backward: x = d(out) [B, C] -> out [B*n, C]."""
    tok = out if backward else x
    vec = x if backward else out
    _rowmajor(tok, "segment_mean: token rows")
    _require(vec.dim() == 2, "segment_mean: [B, C] is required")
    Cc = vec.shape[1]
    _dense(vec, "segment_mean: [B, C]", _F32, B * Cc)
    _require(tok.dtype == torch.float32 and tok.shape[0] == B * n and tok.shape[1] == Cc,
             f"segment_mean: token rows {tuple(tok.shape)} {tok.dtype}, expected fp32 [{B * n}, {Cc}]")
    if backward:
        check(lib().uia_segment_mean_bwd(_stream(), B, n, Cc, _p(x), _p(out), out.stride(0)), "uia_segment_mean_bwd")
    else:
        check(lib().uia_segment_mean_fwd(_stream(), B, n, Cc, _p(x), x.stride(0), _p(out)), "uia_segment_mean_fwd")


def dicece_fwd_bwd(logits, label, smooth_nr=1e-8, smooth_dr=1e-8, out=None):
    """logits fp32 [B,C,H,W], label [B,1,H,W] (class indices) -> (loss 0-dim fp32, dlogits fp32 [B,C,H,W]).
    out: an optional (loss, dlogits) pair of fp32 tensors (1 and B·C·H·W elements) to write into instead of new ones."""
    _require(logits.dim() == 4, "dicece_fwd_bwd: logits [B, C, H, W] are required")
    _dense(logits, "dicece_fwd_bwd: logits", _F32)
    B, Cc, H, W = logits.shape
    _require(label.numel() == B * H * W, f"dicece_fwd_bwd: label has {label.numel()} elements, expected {B * H * W}")
    lab = label.reshape(B, H * W).to(torch.float32).contiguous()
    ws = torch.empty(lib().uia_dicece_workspace_bytes(B) // 4, device=logits.device, dtype=torch.float32)
    if out is None:
        loss, dl = torch.empty((), device=logits.device, dtype=torch.float32), torch.empty_like(logits)
    else:
        loss, dl = _dense(out[0], "dicece_fwd_bwd: loss", _F32, 1), _dense(out[1], "dicece_fwd_bwd: dlogits", _F32, logits.numel())
    check(lib().uia_dicece_fwd_bwd(_stream(), B, Cc, H * W, _p(logits), _p(lab), smooth_nr, smooth_dr, _p(ws), _p(loss), _p(dl)), "uia_dicece_fwd_bwd")
    return loss, dl


def focal_fwd_bwd(logits, labels, gamma=2.0, alpha=None):
    """logits fp32 [N,C], labels int64 [N] -> (loss 0-dim fp32 = mean over N·C of MONAI's sigmoid focal term, dlogits fp32 [N,C] = d loss / d logits).
    alpha None: no class weighting.  A label outside [0, C) makes the loss NaN."""
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
    N, Cc = logits.shape
    lab = labels.reshape(N).to(torch.int64).contiguous()
    ws = torch.empty(lib().uia_focal_workspace_bytes(N, Cc), device=logits.device, dtype=torch.uint8)
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    dl = torch.empty_like(logits)
    check(lib().uia_focal_fwd_bwd(_stream(), N, Cc, _p(logits), _p(lab), float(gamma), -1.0 if alpha is None else float(alpha), _p(ws), ws.numel(),
                                  _p(loss), _p(dl)), "uia_focal_fwd_bwd")
    return loss, dl


def binary_cls_stats(p1, labels):
    """p1 fp32 [N] (probability of class 1), labels int64 [N] in {0, 1} -> fp64 device record [5]: TP, FP, TN, FN at p1 > 0.5 and the tie-aware AUROC.
    The sort is plumbing (torch.sort on the device); the grouped rank sum and the counts are the kernel's."""
    p1 = p1.reshape(-1).to(torch.float32).contiguous()
    lab = labels.reshape(-1).to(torch.int64).contiguous()
    assert p1.numel() == lab.numel() and p1.device == lab.device
    perm = torch.sort(p1, stable=True).indices
    N = p1.numel()
    ws = torch.empty(lib().uia_binary_cls_stats_workspace_bytes(N), device=p1.device, dtype=torch.uint8)
    rec = torch.empty(5, device=p1.device, dtype=torch.float64)
    check(lib().uia_binary_cls_stats(_stream(), N, _p(p1), _p(lab), _p(perm), _p(ws), ws.numel(), _p(rec)), "uia_binary_cls_stats")
    return rec


def binary_roc_curve(p1, labels):
    """p1 fp32 [N], labels int64 [N] in {0, 1} -> (count int32 [1], fpr fp64 [N+1], tpr fp64 [N+1], thr fp32 [N+1]) device tensors: the exact ROC curve as
    torchmetrics ROC(task="binary", thresholds=None) gives it.  Point 0 is (0, 0, 1.0), then one point per distinct score, descending; the first `count`
    entries are the curve (the caller reads count, once; -1: a label outside {0, 1} or a NaN score).  The sort is plumbing, as in binary_cls_stats."""
    p1 = p1.reshape(-1).to(torch.float32).contiguous()
    lab = labels.reshape(-1).to(torch.int64).contiguous()
    assert p1.numel() == lab.numel() and p1.device == lab.device
    perm = torch.sort(p1, stable=True).indices
    N = p1.numel()
    ws = torch.empty(max(lib().uia_binary_roc_curve_workspace_bytes(N), 16), device=p1.device, dtype=torch.uint8)
    count = torch.zeros(1, device=p1.device, dtype=torch.int32)
    fpr = torch.zeros(N + 1, device=p1.device, dtype=torch.float64)
    tpr = torch.zeros(N + 1, device=p1.device, dtype=torch.float64)
    thr = torch.zeros(N + 1, device=p1.device, dtype=torch.float32)
    check(lib().uia_binary_roc_curve(_stream(), N, _p(p1), _p(lab), _p(perm), _p(ws), ws.numel(), _p(count), _p(fpr), _p(tpr), _p(thr)),
          "uia_binary_roc_curve")
    return count, fpr, tpr, thr


def zero_shot_score(img, prompts, class_off, out=None, row=0, want_probs=True, want_normalized=False):
    """img [N, E] raw image features, prompts [T, E] raw text features of every prompt, class after class (non-fp32 is converted); class_off a host
    sequence of C + 1 ints, class c owning the prompt rows class_off[c] .. class_off[c+1]-1 -> (logits, probs, img_n).  logits[i, c] is the mean over the
    class's prompts of 100 · <img_i / ||img_i||, prompt_t / ||prompt_t||> (no eps), bit for bit independent of the batch the row arrives in.  out: a
    contiguous fp32 [M, C] buffer that takes the rows [row, row + N) (a whole split in one buffer); logits is then that view.  probs fp32 [N, C] (softmax)
    unless want_probs is False, img_n fp32 [N, E] (the normalised rows) only if want_normalized; None otherwise.  Enqueued only: nothing is read back."""
    _p(img), _p(prompts)                                          # CPU tensors are refused before anything else
    _require(img.dim() == 2 and prompts.dim() == 2 and img.shape[1] == prompts.shape[1] and img.device == prompts.device,
             f"zero_shot_score: img {tuple(img.shape)} and prompts {tuple(prompts.shape)} must be [N, E] and [T, E] on one device")
    a, b = img.detach().float().contiguous(), prompts.detach().float().contiguous()
    (N, E), T = a.shape, b.shape[0]
    off = [int(v) for v in (class_off.tolist() if isinstance(class_off, torch.Tensor) else class_off)]
    Cc, row = len(off) - 1, int(row)
    _require(Cc >= 1, "zero_shot_score: class_off needs at least two entries")
    if out is None:
        _require(row == 0, "zero_shot_score: a row offset needs an out buffer")
        out = torch.empty(N, Cc, device=a.device, dtype=torch.float32)
    _dense(out, "zero_shot_score: out", _F32)
    _require(out.dim() == 2 and out.shape[1] == Cc and out.device == a.device and 0 <= row and row + N <= out.shape[0],
             f"zero_shot_score: out {tuple(out.shape)} cannot take rows [{row}, {row + N}) of {Cc} classes")
    probs = torch.empty(N, Cc, device=a.device, dtype=torch.float32) if want_probs else None
    img_n = torch.empty(N, E, device=a.device, dtype=torch.float32) if want_normalized else None
    offs = (C.c_int32 * (Cc + 1))(*off)
    check(lib().uia_zero_shot_score(_stream(), N, T, E, Cc, offs, _p(a), _p(b), _p(out), Cc, row, _p(probs), _p(img_n)), "uia_zero_shot_score")
    return out[row:row + N], probs, img_n


def surface_distances(logits, label, percentile=95.0):
    """logits [B,2,H,W] (non-fp32 is converted), label [B,1,H,W] -> (hd, asd) fp64 device tensors [B]: MONAI's percentile Hausdorff distance (symmetric) and
    average surface distance (P -> G) of the arg-max mask against label > 0, in pixels; NaN where either mask is empty.  Enqueued only: nothing is read back."""
    assert logits.dim() == 4 and logits.shape[1] == 2, f"surface_distances: logits must be [B, 2, H, W], got {tuple(logits.shape)}"
    B, _, H, W = logits.shape
    assert label.numel() == B * H * W and label.device == logits.device, f"surface_distances: label {tuple(label.shape)} does not match logits {tuple(logits.shape)}"
    lg = logits.float().contiguous()
    lab = label.reshape(B, 1, H, W).to(torch.float32).contiguous()
    ws = torch.empty(lib().uia_surface_distances_workspace_bytes(B, H, W), device=lg.device, dtype=torch.uint8)
    hd = torch.empty(B, device=lg.device, dtype=torch.float64)
    asd = torch.empty(B, device=lg.device, dtype=torch.float64)
    check(lib().uia_surface_distances(_stream(), B, H, W, _p(lg), _p(lab), float(percentile), _p(ws), ws.numel(), _p(hd), _p(asd)), "uia_surface_distances")
    return hd, asd


_SEG_LABEL = {torch.uint8: 0, torch.float32: 1}


def _seg_viz_args(logits, images, labels, mask_rgb, overlay_rgb, pred):
    _p(logits), _p(images), _p(labels)                            # CPU tensors are refused before anything else
    _require(logits.dim() == 4 and logits.shape[2] == logits.shape[3], f"seg_viz: logits must be [B, C, S, S], got {tuple(logits.shape)}")
    B, Cc, S, _ = logits.shape
    _dense(logits, "seg_viz: logits", _F32)
    _dense(images, "seg_viz: images", _F32)
    _require(images.dim() == 4 and images.shape[0] == B and tuple(images.shape[2:]) == (S, S),
             f"seg_viz: images {tuple(images.shape)} do not match logits {tuple(logits.shape)}")
    _dense(labels, "seg_viz: labels", tuple(_SEG_LABEL), numel=B * S * S)
    for t, name, n in ((mask_rgb, "mask_rgb", 3), (overlay_rgb, "overlay_rgb", 3), (pred, "pred", 1)):
        _dense(t, f"seg_viz: {name}", (torch.uint8,), numel=B * S * S * n)
        _require(t.device == logits.device, f"seg_viz: {name} is on {t.device}, logits on {logits.device}")
    return B, Cc, images.shape[1], S, _SEG_LABEL[labels.dtype]


def seg_viz_form(logits, images, labels, mask_rgb, overlay_rgb, pred):
    """1 when seg_viz of these tensors runs on the four-pixels-per-thread kernel, 0 for the pixel-per-thread one (uia_seg_viz_form: size and addresses only)."""
    _, _, _, S, code = _seg_viz_args(logits, images, labels, mask_rgb, overlay_rgb, pred)
    return int(lib().uia_seg_viz_form(S, code, _p(logits), _p(images), _p(labels), _p(mask_rgb), _p(overlay_rgb), _p(pred)))


def seg_viz(logits, images, labels, mask_rgb=None, overlay_rgb=None, pred=None):
    """logits fp32 [B,2,S,S], images fp32 [B,1|3,S,S] (channel 0 is drawn), labels uint8 or fp32 [B,1,S,S], all contiguous -> (mask_rgb [B,S,S,3],
    overlay_rgb [B,S,S,3], pred [B,S,S]), uint8: ground truth red and prediction green, the same over the grey input, and the binary mask, with the
    arg-max rule of the Dice / IoU / surface metrics.  The outputs may be passed in (contiguous uint8 of those sizes).  Enqueued only: nothing is read back."""
    if mask_rgb is None:
        B, _, S, _ = logits.shape
        mask_rgb, overlay_rgb = (torch.empty(B, S, S, 3, device=logits.device, dtype=torch.uint8) for _ in range(2))
        pred = torch.empty(B, S, S, device=logits.device, dtype=torch.uint8)
    B, Cc, Ci, S, code = _seg_viz_args(logits, images, labels, mask_rgb, overlay_rgb, pred)
    check(lib().uia_seg_viz(_stream(), B, Cc, Ci, S, _p(logits), _p(images), _p(labels), code, _p(mask_rgb), _p(overlay_rgb), _p(pred)), "uia_seg_viz")
    return mask_rgb, overlay_rgb, pred


def retrieval_ranks(img, txt, normalize=True):
    """img, txt [N, E] paired features (non-fp32 is converted) -> (gt_i2t, eq_i2t, gt_t2i, eq_t2i), int32 device tensors [N]: for each query the number of
    OTHER candidates scoring strictly above / exactly equal to its own pair, s_ij = <img_i, txt_j> on the exact fp32 MFMA (rows L2-normalised first when
    `normalize`).  The N x N score matrix is never formed.  Enqueued only: nothing is read back."""
    _p(img), _p(txt)                                              # CPU tensors are refused before anything else
    assert img.dim() == 2 and img.shape == txt.shape and img.device == txt.device, f"retrieval_ranks: img {tuple(img.shape)} and txt {tuple(txt.shape)} must be paired [N, E]"
    a, b = img.detach().float().contiguous(), txt.detach().float().contiguous()
    N, E = a.shape
    ws = torch.empty(lib().uia_retrieval_workspace_bytes(N, E), device=a.device, dtype=torch.uint8)
    out = torch.empty(4, N, device=a.device, dtype=torch.int32)
    check(lib().uia_retrieval_ranks(_stream(), N, E, _p(a), _p(b), 1 if normalize else 0, _p(ws), ws.numel(), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3])),
          "uia_retrieval_ranks")
    return out[0], out[1], out[2], out[3]


def retrieval_topk(queries, gallery, k, normalize=True, splits=0):
    """queries [Q, E], gallery [N, E] (non-fp32 is converted), 1 <= k <= min(N, 32) -> (idx int32 [Q, k], score fp32 [Q, k]) device tensors: for each query
    its k best gallery rows, score descending, equal scores by gallery index ascending, NaN scores last; the same score bits as retrieval_ranks.  The
    Q x N score matrix is never formed.  splits: gallery strips per row tile, 0 = the kernel's rule (the result does not depend on it).  Enqueued only."""
    _p(queries), _p(gallery)                                      # CPU tensors are refused before anything else
    assert queries.dim() == 2 and gallery.dim() == 2 and queries.shape[1] == gallery.shape[1] and queries.device == gallery.device, \
        f"retrieval_topk: queries {tuple(queries.shape)} and gallery {tuple(gallery.shape)} must be [Q, E] and [N, E] on one device"
    a, b = queries.detach().float().contiguous(), gallery.detach().float().contiguous()
    (Q, E), N, K = a.shape, b.shape[0], int(k)
    need = lib().uia_retrieval_topk_workspace_bytes(Q, N, E, K)
    ws = torch.empty(max(need, 16), device=a.device, dtype=torch.uint8)        # need == 0: a shape outside the limits, which the call below names
    idx = torch.empty(Q, max(K, 0), device=a.device, dtype=torch.int32)
    score = torch.empty(Q, max(K, 0), device=a.device, dtype=torch.float32)
    check(lib().uia_retrieval_topk(_stream(), Q, N, E, K, _p(a), _p(b), 1 if normalize else 0, int(splits), _p(ws), need, _p(idx), _p(score)),
          "uia_retrieval_topk")
    return idx, score


def retrieval_stats(gt, k_values):
    """gt int32 [N] (one direction of retrieval_ranks), k_values a sequence of K -> fp64 device record [len(k_values) + 2]: R@K in percent for each K, the
    median and the mean of rank = 1 + gt."""
    g = gt.reshape(-1).to(torch.int32).contiguous()
    ks = (C.c_int32 * len(k_values))(*[int(k) for k in k_values])
    N = g.numel()
    pg = _p(g)
    ws = torch.empty(lib().uia_retrieval_stats_workspace_bytes(N), device=g.device, dtype=torch.uint8)
    rec = torch.empty(len(k_values) + 2, device=g.device, dtype=torch.float64)
    check(lib().uia_retrieval_stats(_stream(), N, pg, len(k_values), ks, _p(ws), ws.numel(), _p(rec)), "uia_retrieval_stats")
    return rec


# ---------------------------------------------------------------- training-time augmentation (csrc/augment.hip)
AUG_MAX_OPS, AUG_ROWS = 13, 14             # ops per image; rows of an image in the program table (row 0: n, with_mask, 0, 0)


def augment_workspace(B, S, device):
    """The scratch of one uia_augment_batch call on [B, 1, S, S] (a caller that augments every batch keeps it)."""
    need = lib().uia_augment_workspace_bytes(int(B), int(S))
    if need == 0:
        raise UiaError(f"augment_batch: shape B={B} S={S} is outside the kernel's limits (1 <= B <= 65535, 8 <= S <= 1024)")
    return torch.empty(need, device=device, dtype=torch.uint8)


def augment_batch(images, masks, programs, out_images=None, out_masks=None, ws=None):
    """images fp32 [B, 1, S, S] in [0, 1] and masks uint8 [B, 1, S, S] (or None) on the device, programs a HOST int32 tensor [B, 14, 4]
    (src/datasets/augment.draw_programs; pinned memory makes its copy asynchronous, and it must then stay unchanged until the copy has run) ->
    (out_images, out_masks): every image run through its program in one launch; an image with an empty program is copied bit for bit.
    Enqueued only: nothing is read back.  out_* and ws may be handed in to be reused."""
    _p(images), _p(masks)                                         # CPU tensors are refused before anything else
    if images.dim() != 4 or images.shape[1] != 1 or images.shape[2] != images.shape[3] or images.dtype != torch.float32 or not images.is_contiguous():
        raise UiaError(f"augment_batch: images must be contiguous fp32 [B, 1, S, S], got {images.dtype} {tuple(images.shape)}")
    B, _, S, _ = images.shape
    if masks is not None and (masks.shape != images.shape or masks.dtype != torch.uint8 or not masks.is_contiguous() or masks.device != images.device):
        raise UiaError(f"augment_batch: masks must be contiguous uint8 {tuple(images.shape)} beside the images, got {masks.dtype} {tuple(masks.shape)}")
    if (not isinstance(programs, torch.Tensor) or programs.is_cuda or programs.dtype != torch.int32 or tuple(programs.shape) != (B, AUG_ROWS, 4)
            or not programs.is_contiguous()):
        raise UiaError(f"augment_batch: programs must be a contiguous host int32 tensor [{B}, {AUG_ROWS}, 4]")
    if out_images is None:
        out_images = torch.empty_like(images)
    if masks is not None and out_masks is None:
        out_masks = torch.empty_like(masks)
    if masks is None:
        out_masks = None
    for o, i, name in ((out_images, images, "out_images"), (out_masks, masks, "out_masks")):
        if i is not None and (o.shape != i.shape or o.dtype != i.dtype or not o.is_contiguous() or o.device != i.device):
            raise UiaError(f"augment_batch: {name} must match its input ({i.dtype} {tuple(i.shape)}, contiguous, same device)")
    if ws is None:
        ws = augment_workspace(B, S, images.device)
    check(lib().uia_augment_batch(_stream(), B, S, _p(images), _p(masks), programs.data_ptr(), _p(ws), ws.numel(), _p(out_images), _p(out_masks)),
          "uia_augment_batch")
    return out_images, out_masks


def augment_gather(images, masks, programs, out_images=None, out_masks=None, ws=None):
    """augment_batch on a device-resident set: images [N, 1, S, S], fp32 in [0, 1] or uint8 (the 8-bit plane as stored), masks uint8 [N, 1, S, S]
    or None, programs a HOST int32 tensor [B, 14, 4] whose row 0 of output b is (n, with_mask, src, 0): output b is resident row src run through its
    program (n == 0: the row itself; bytes as u / 255) -> (out_images fp32 [B, 1, S, S], out_masks uint8 [B, 1, S, S] or None).  One table copy and
    one launch; equal, bit for bit, to augment_batch(images[src] (bytes: .float() / 255), programs).  Rows may repeat and B may exceed N."""
    _p(images), _p(masks)
    if (images.dim() != 4 or images.shape[1] != 1 or images.shape[2] != images.shape[3] or images.dtype not in (torch.float32, torch.uint8)
            or not images.is_contiguous() or images.shape[0] < 1):
        raise UiaError(f"augment_gather: images must be contiguous fp32 or uint8 [N, 1, S, S], got {images.dtype} {tuple(images.shape)}")
    N, _, S, _ = images.shape
    if masks is not None and (masks.shape != images.shape or masks.dtype != torch.uint8 or not masks.is_contiguous() or masks.device != images.device):
        raise UiaError(f"augment_gather: masks must be contiguous uint8 {tuple(images.shape)} beside the images, got {masks.dtype} {tuple(masks.shape)}")
    if (not isinstance(programs, torch.Tensor) or programs.is_cuda or programs.dtype != torch.int32 or programs.dim() != 3
            or tuple(programs.shape[1:]) != (AUG_ROWS, 4) or programs.shape[0] < 1 or not programs.is_contiguous()):
        raise UiaError(f"augment_gather: programs must be a contiguous host int32 tensor [B, {AUG_ROWS}, 4]")
    B = programs.shape[0]
    if out_images is None:
        out_images = torch.empty((B, 1, S, S), dtype=torch.float32, device=images.device)
    if masks is not None and out_masks is None:
        out_masks = torch.empty((B, 1, S, S), dtype=torch.uint8, device=images.device)
    if masks is None:
        out_masks = None
    for o, dt, name in ((out_images, torch.float32, "out_images"), (out_masks, torch.uint8, "out_masks")):
        if o is not None and (tuple(o.shape) != (B, 1, S, S) or o.dtype != dt or not o.is_contiguous() or o.device != images.device):
            raise UiaError(f"augment_gather: {name} must be contiguous {dt} [{B}, 1, {S}, {S}] on the images' device")
    if ws is None:
        ws = augment_workspace(B, S, images.device)
    check(lib().uia_augment_gather(_stream(), N, B, S, 1 if images.dtype == torch.uint8 else 0, _p(images), _p(masks), programs.data_ptr(), _p(ws),
                                   ws.numel(), _p(out_images), _p(out_masks)), "uia_augment_gather")
    return out_images, out_masks


# ---------------------------------------------------------------- Pillow's resize of a ragged batch (csrc/resize.hip)
RESIZE_DESC = 8                            # int32 per image: offset, H, W, mask offset or -1, dst_h, dst_w, y0, x0


def resize_workspace(B, device):
    """The scratch of one uia_resize_batch call on B images (a caller that resizes every batch keeps it)."""
    need = lib().uia_resize_workspace_bytes(int(B))
    if need == 0:
        raise UiaError(f"resize_batch: B={B} is outside the kernel's limits (1 <= B <= 65535)")
    return torch.empty(need, device=device, dtype=torch.uint8)


def resize_batch(src, desc, S, C=1, out_images=None, out_masks=None, ws=None):
    """src: a 1-D uint8 device tensor holding B decoded images back to back (8 bits per channel, C interleaved channels, any offsets) and their
    one-byte-per-pixel masks; desc a HOST int32 tensor [B, 8], per image (offset, H, W, mask offset or -1, dst_h, dst_w, y0, x0) (pinned memory makes
    its copy asynchronous, and it must then stay unchanged until the copy has run) -> (out_images fp32 [B, C, S, S], out_masks uint8 [B, 1, S, S] or
    None when no image has a mask): every image resampled to dst_h x dst_w as PIL's `Image.resize` does it (antialiased bicubic; masks: nearest), the
    S x S window at (y0, x0) written as q / 255, in one launch.  Enqueued only.  out_* and ws may be handed in to be reused."""
    _p(src)
    if src.dim() != 1 or src.dtype != torch.uint8 or not src.is_contiguous():
        raise UiaError(f"resize_batch: src must be a contiguous 1-D uint8 tensor, got {src.dtype} {tuple(src.shape)}")
    if (not isinstance(desc, torch.Tensor) or desc.is_cuda or desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != RESIZE_DESC
            or desc.shape[0] < 1 or not desc.is_contiguous()):
        raise UiaError(f"resize_batch: desc must be a contiguous host int32 tensor [B, {RESIZE_DESC}]")
    B, S, C = desc.shape[0], int(S), int(C)
    with_masks = out_masks is not None or bool((desc[:, 3] >= 0).any())
    if out_images is None:
        out_images = torch.empty((B, C, S, S), dtype=torch.float32, device=src.device)
    if with_masks and out_masks is None:
        out_masks = torch.empty((B, 1, S, S), dtype=torch.uint8, device=src.device)
    for o, ch, dt, name in ((out_images, C, torch.float32, "out_images"), (out_masks, 1, torch.uint8, "out_masks")):
        if o is not None and (tuple(o.shape) != (B, ch, S, S) or o.dtype != dt or not o.is_contiguous() or o.device != src.device):
            raise UiaError(f"resize_batch: {name} must be contiguous {dt} [{B}, {ch}, {S}, {S}] on the source's device")
    if ws is None:
        ws = resize_workspace(B, src.device)
    check(lib().uia_resize_batch(_stream(), B, C, S, _p(src), src.numel(), desc.data_ptr(), _p(ws), ws.numel(), _p(out_images), _p(out_masks)),
          "uia_resize_batch")
    return out_images, out_masks


def resize_batch_rgb(src, desc, S, out_images=None, ws=None):
    """resize_batch for a batch that mixes gray and colour images: word 3 of an image's descriptor is its channel count, 1 or 3, (offset, H, W, channels,
    dst_h, dst_w, y0, x0) -> out_images fp32 [B, 3, S, S]; a one-channel image is resampled once and written to all three planes (PIL's convert("RGB") of
    an "L" image, then the resize).  No masks.  Enqueued only; out_images and ws may be handed in to be reused."""
    _p(src)
    if src.dim() != 1 or src.dtype != torch.uint8 or not src.is_contiguous():
        raise UiaError(f"resize_batch_rgb: src must be a contiguous 1-D uint8 tensor, got {src.dtype} {tuple(src.shape)}")
    if (not isinstance(desc, torch.Tensor) or desc.is_cuda or desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != RESIZE_DESC
            or desc.shape[0] < 1 or not desc.is_contiguous()):
        raise UiaError(f"resize_batch_rgb: desc must be a contiguous host int32 tensor [B, {RESIZE_DESC}]")
    B, S = desc.shape[0], int(S)
    if out_images is None:
        out_images = torch.empty((B, 3, S, S), dtype=torch.float32, device=src.device)
    if tuple(out_images.shape) != (B, 3, S, S) or out_images.dtype != torch.float32 or not out_images.is_contiguous() or out_images.device != src.device:
        raise UiaError(f"resize_batch_rgb: out_images must be contiguous {torch.float32} [{B}, 3, {S}, {S}] on the source's device")
    if ws is None:
        ws = resize_workspace(B, src.device)
    check(lib().uia_resize_batch_rgb(_stream(), B, S, _p(src), src.numel(), desc.data_ptr(), _p(ws), ws.numel(), _p(out_images)), "uia_resize_batch_rgb")
    return out_images


# ---------------------------------------------------------------- native-size masks from S x S logits (csrc/seg_native.hip)
SEG_NATIVE_DESC = 8                        # int32 per image: source offset or -1, H, W, mask offset in out, overlay offset in out or -1, 0, 0, 0
SEG_NATIVE_EMPTY = (0, 2 ** 31 - 1, 2 ** 31 - 1, -1, -1, 0, 0, 0)      # the stats row of an empty mask
_SEG_NATIVE_WS = {}


def seg_native_workspace(B, device):
    """The scratch of uia_seg_predict_native on B images, kept per (device, stream, B): launches of one stream are ordered, so they may share it."""
    need = lib().uia_seg_native_workspace_bytes(int(B))
    if need == 0:
        raise UiaError(f"seg_predict_native: B={B} is outside the kernel's limits (1 <= B <= 65535)")
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream, int(B))
    ws = _SEG_NATIVE_WS.get(key)
    if ws is None:
        ws = _SEG_NATIVE_WS[key] = torch.empty(need, device=device, dtype=torch.uint8)
    return ws


def seg_predict_native(logits, src, desc, out, stats=None):
    """logits fp32 [B, 2, S, S] on the device; src the batch's ragged 1-D uint8 device buffer (the one resize_batch read) or None when no image asks for an
    overlay; desc a HOST int32 tensor [B, 8], per image (source offset or -1, H, W, mask offset in out, overlay offset in out or -1, 0, 0, 0) (pinned memory
    makes its copy asynchronous, and it must then stay unchanged until the copy has run); out a 1-D uint8 device buffer -> stats int32 [B, 8] on the
    device, per image (foreground pixels, ymin, xmin, ymax, xmax, 0, 0, 0) — SEG_NATIVE_EMPTY for an empty mask.  One launch writes into `out` every
    image's H x W mask (255 where class 1 wins the bilinearly upsampled logits, torch's arg-max rule) and, where both offsets are given, its H x W x 3
    overlay (g, max(g, p), g).  Enqueued only: nothing is read back."""
    _p(logits), _p(src), _p(out), _p(stats)
    if logits.dim() != 4 or logits.shape[1] != 2 or logits.shape[2] != logits.shape[3] or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise UiaError(f"seg_predict_native: logits must be contiguous fp32 [B, 2, S, S], got {logits.dtype} {tuple(logits.shape)}")
    B, _, S, _ = logits.shape
    for t, name in ((src, "src"), (out, "out")):
        if t is not None and (t.dim() != 1 or t.dtype != torch.uint8 or not t.is_contiguous() or t.device != logits.device):
            raise UiaError(f"seg_predict_native: {name} must be a contiguous 1-D uint8 tensor on the logits' device, got {t.dtype} {tuple(t.shape)}")
    if out is None:
        raise UiaError("seg_predict_native: out is required (the caller lays the masks and overlays out in it)")
    if (not isinstance(desc, torch.Tensor) or desc.is_cuda or desc.dtype != torch.int32 or tuple(desc.shape) != (B, SEG_NATIVE_DESC) or not desc.is_contiguous()):
        raise UiaError(f"seg_predict_native: desc must be a contiguous host int32 tensor [{B}, {SEG_NATIVE_DESC}]")
    if stats is None:
        stats = torch.empty((B, SEG_NATIVE_DESC), dtype=torch.int32, device=logits.device)
    if tuple(stats.shape) != (B, SEG_NATIVE_DESC) or stats.dtype != torch.int32 or not stats.is_contiguous() or stats.device != logits.device:
        raise UiaError(f"seg_predict_native: stats must be contiguous int32 [{B}, {SEG_NATIVE_DESC}] on the logits' device")
    ws = seg_native_workspace(B, logits.device)
    check(lib().uia_seg_predict_native(_stream(), B, S, _p(logits), _p(src), 0 if src is None else src.numel(), desc.data_ptr(), _p(out), out.numel(), _p(ws),
                                       ws.numel(), _p(stats)), "uia_seg_predict_native")
    return stats


# ---------------------------------------------------------------- the same for an ensemble of K members (csrc/seg_native_ens.hip)
SEG_NATIVE_ENS_MAX_K = 16
_SEG_NATIVE_ENS_WS = {}


def seg_native_ens_workspace(B, device):
    """The scratch of uia_seg_predict_native_ens on B images, kept per (device, stream, B): launches of one stream are ordered, so they may share it."""
    need = lib().uia_seg_native_ens_workspace_bytes(int(B))
    if need == 0:
        raise UiaError(f"seg_predict_native_ens: B={B} is outside the kernel's limits (1 <= B <= 65535)")
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream, int(B))
    ws = _SEG_NATIVE_ENS_WS.get(key)
    if ws is None:
        ws = _SEG_NATIVE_ENS_WS[key] = torch.empty(need, device=device, dtype=torch.uint8)
    return ws


def seg_flip_bits(flips):
    """A sequence of K values 0 .. 3 (1: the member saw the horizontally flipped input, 2: the vertically flipped one, 3: both) -> the `flips` word of
    uia_seg_predict_native_ens, two bits per member."""
    flips = [int(f) for f in flips]
    if not 1 <= len(flips) <= SEG_NATIVE_ENS_MAX_K or any(f not in (0, 1, 2, 3) for f in flips):
        raise UiaError(f"seg_predict_native_ens: flips must be 1 .. {SEG_NATIVE_ENS_MAX_K} values 0 .. 3, one per member, got {flips}")
    word = 0
    for k, f in enumerate(flips):
        word |= f << (2 * k)
    return word


def seg_predict_native_ens(logits, flips, src, desc, out, threshold=0.5, stats=None, sums=None):
    """seg_predict_native for K members: logits fp32 [K, B, 2, S, S] on the device, flips a sequence of K values 0 .. 3 (bit 0: member k's logits are of
    the horizontally flipped S x S input, bit 1: of the vertically flipped one; the kernel un-flips while it reads); src and out as seg_predict_native's;
    desc a HOST int32 tensor [B, 8], per image (source offset or -1, H, W, mask offset, overlay offset or -1, probability offset or -1, spread offset or -1,
    0) -> (stats int32 [B, 8], sums int64 [B, 2]) on the device.  One launch writes every image's mask (255 where the members' mean foreground
    probability P > threshold), its overlay, q = (uint8)(255 P + 0.5) at the probability offset and r = (uint8)(255 (max_k p_k - min_k p_k) + 0.5) at the
    spread offset; sums = (sum of q over the mask, sum of r over the image).  A pixel with a NaN member: mask 0, q 0, r 255.  Enqueued only."""
    _p(logits), _p(src), _p(out), _p(stats), _p(sums)
    if logits.dim() != 5 or logits.shape[2] != 2 or logits.shape[3] != logits.shape[4] or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise UiaError(f"seg_predict_native_ens: logits must be contiguous fp32 [K, B, 2, S, S], got {logits.dtype} {tuple(logits.shape)}")
    K, B, _, S, _ = logits.shape
    flips = list(flips)
    word = seg_flip_bits(flips)
    if len(flips) != K:
        raise UiaError(f"seg_predict_native_ens: {len(flips)} flips for {K} members")
    threshold = float(threshold)
    if not 0.0 < threshold < 1.0:
        raise UiaError(f"seg_predict_native_ens: threshold {threshold} (0 < threshold < 1)")
    for t, name in ((src, "src"), (out, "out")):
        if t is not None and (t.dim() != 1 or t.dtype != torch.uint8 or not t.is_contiguous() or t.device != logits.device):
            raise UiaError(f"seg_predict_native_ens: {name} must be a contiguous 1-D uint8 tensor on the logits' device, got {t.dtype} {tuple(t.shape)}")
    if out is None:
        raise UiaError("seg_predict_native_ens: out is required (the caller lays the masks, overlays and maps out in it)")
    if (not isinstance(desc, torch.Tensor) or desc.is_cuda or desc.dtype != torch.int32 or tuple(desc.shape) != (B, SEG_NATIVE_DESC) or not desc.is_contiguous()):
        raise UiaError(f"seg_predict_native_ens: desc must be a contiguous host int32 tensor [{B}, {SEG_NATIVE_DESC}]")
    if stats is None:
        stats = torch.empty((B, SEG_NATIVE_DESC), dtype=torch.int32, device=logits.device)
    if tuple(stats.shape) != (B, SEG_NATIVE_DESC) or stats.dtype != torch.int32 or not stats.is_contiguous() or stats.device != logits.device:
        raise UiaError(f"seg_predict_native_ens: stats must be contiguous int32 [{B}, {SEG_NATIVE_DESC}] on the logits' device")
    if sums is None:
        sums = torch.empty((B, 2), dtype=torch.int64, device=logits.device)
    if tuple(sums.shape) != (B, 2) or sums.dtype != torch.int64 or not sums.is_contiguous() or sums.device != logits.device:
        raise UiaError(f"seg_predict_native_ens: sums must be contiguous int64 [{B}, 2] on the logits' device")
    ws = seg_native_ens_workspace(B, logits.device)
    check(lib().uia_seg_predict_native_ens(_stream(), K, B, S, _p(logits), word, threshold, _p(src), 0 if src is None else src.numel(), desc.data_ptr(), _p(out),
                                           out.numel(), _p(ws), ws.numel(), _p(stats), _p(sums)), "uia_seg_predict_native_ens")
    return stats, sums


# ---------------------------------------------------------------- connected components of native-size masks (csrc/components.hip)
MASK_COMPONENTS_DESC = 8                   # int32 per image: mask offset, H, W, overlay offset or -1, min_area, keep, connectivity (4 | 8), 0
MASK_COMPONENTS_MAX_LIST = 32
_MASK_COMPONENTS_WS = {}


def mask_components_workspace(B, pixels, device):
    """The scratch of uia_mask_components on B images of `pixels` pixels in all, kept per (device, stream) and grown when a batch needs more: launches of
    one stream are ordered, so they may share it."""
    need = lib().uia_mask_components_workspace_bytes(int(B), int(pixels))
    if need == 0:
        raise UiaError(f"mask_components: B={B}, pixels={pixels} is outside the kernel's limits (1 <= B <= 65535, 1 <= pixels < 2^31)")
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    ws = _MASK_COMPONENTS_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _MASK_COMPONENTS_WS[key] = torch.empty(need + need // 4, device=device, dtype=torch.uint8)
    return ws


def mask_components(buf, desc, max_list=0):
    """buf a 1-D uint8 device buffer holding the batch's masks (and overlays), e.g. the `out` of seg_predict_native; desc a HOST int32 tensor [B, 8], per
    image (mask offset, H, W, overlay offset or -1, min_area, keep, connectivity, 0) (pinned memory makes its copy asynchronous, and it must then stay
    unchanged until the copy has run) -> (stats int32 [B, 8], list int32 [B, max_list, 8]) on the device.  In place: every pixel of a 4- / 8-connected
    component that is not kept (area >= min_area, and among the `keep` largest when keep > 0; equal areas by first pixel) gets mask byte 0 and its
    overlay's green byte the red one.  stats = (foreground after, ymin, xmin, ymax, xmax, components found, components kept, foreground before); list rows
    = (area, ymin, xmin, ymax, xmax, first pixel, cy, cx) of the first max_list kept components, largest first, unused rows zero.  Enqueued only."""
    _p(buf)
    if buf is None or buf.dim() != 1 or buf.dtype != torch.uint8 or not buf.is_contiguous() or not buf.is_cuda:
        raise UiaError("mask_components: buf must be a contiguous 1-D uint8 tensor on the device")
    if (not isinstance(desc, torch.Tensor) or desc.is_cuda or desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != MASK_COMPONENTS_DESC
            or desc.shape[0] < 1 or not desc.is_contiguous()):
        raise UiaError(f"mask_components: desc must be a contiguous host int32 tensor [B, {MASK_COMPONENTS_DESC}]")
    max_list = int(max_list)
    if not 0 <= max_list <= MASK_COMPONENTS_MAX_LIST:
        raise UiaError(f"mask_components: max_list={max_list} (0 .. {MASK_COMPONENTS_MAX_LIST})")
    B = desc.shape[0]
    pixels = int((desc[:, 1].long().clamp(min=0) * desc[:, 2].long().clamp(min=0)).sum())
    stats = torch.empty((B, 8), dtype=torch.int32, device=buf.device)
    rows = torch.empty((B, max_list, 8), dtype=torch.int32, device=buf.device)
    ws = mask_components_workspace(B, max(1, min(pixels, 2 ** 31 - 1)), buf.device)     # (a descriptor outside the limits is refused by the launcher, by image)
    check(lib().uia_mask_components(_stream(), B, _p(buf), buf.numel(), desc.data_ptr(), _p(ws), ws.numel(), _p(stats), _p(rows) if max_list else None, max_list),
          "uia_mask_components")
    return stats, rows


# ---------------------------------------------------------------- disk closing / opening and hole filling of native-size masks (csrc/morphology.hip)
MASK_MORPHOLOGY_DESC = 8                   # int32 per image: mask offset, H, W, overlay offset or -1, r_close, r_open, hole_area, hole_connectivity (4 | 8)
MORPHOLOGY_MAX_RADIUS = 64
_MASK_MORPHOLOGY_WS = {}


def mask_morphology_workspace(B, pixels, device):
    """The scratch of uia_mask_morphology on B images of `pixels` pixels in all (10 bytes per pixel), kept per (device, stream) and grown when a batch
    needs more: launches of one stream are ordered, so they may share it."""
    need = lib().uia_mask_morphology_workspace_bytes(int(B), int(pixels))
    _require(need != 0, f"mask_morphology: B={B}, pixels={pixels} is outside the kernel's limits (1 <= B <= 65535, 1 <= pixels < 2^31)")
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    ws = _MASK_MORPHOLOGY_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _MASK_MORPHOLOGY_WS[key] = torch.empty(need + need // 4, device=device, dtype=torch.uint8)
    return ws


def mask_morphology(buf, desc):
    """buf a 1-D uint8 device buffer holding the batch's masks (and overlays), e.g. the `out` of seg_predict_native; desc a HOST int32 tensor [B, 8], per
    image (mask offset, H, W, overlay offset or -1, r_close, r_open, hole_area, hole_connectivity) (pinned memory makes its copy asynchronous, and it
    must then stay unchanged until the copy has run) -> stats int32 [B, 8] on the device.  In place, per image: a closing with the disk of radius r_close
    (0 .. 64), then the holes of the result filled (hole_area -1: every hole, N > 0: holes of at most N pixels, 0: none; a hole is a 4- / 8-connected
    component of the background that does not touch the image's frame), then an opening with the disk of radius r_open; only background inside the
    image erodes.  A new foreground pixel gets mask byte 255 and overlay green 255, a removed one 0 and green = red; every other byte stays.
    stats = (foreground after, ymin, xmin, ymax, xmax, pixels added, pixels removed, foreground before).  Enqueued only."""
    _require(isinstance(buf, torch.Tensor) and buf.is_cuda and buf.dim() == 1, "mask_morphology: buf must be a contiguous 1-D uint8 tensor on the device")
    _dense(buf, "mask_morphology: buf", (torch.uint8,))
    _require(isinstance(desc, torch.Tensor) and not desc.is_cuda and desc.dim() == 2 and desc.shape[1] == MASK_MORPHOLOGY_DESC and desc.shape[0] >= 1,
             f"mask_morphology: desc must be a contiguous host int32 tensor [B, {MASK_MORPHOLOGY_DESC}]")
    _dense(desc, "mask_morphology: desc", (torch.int32,))
    B = desc.shape[0]
    pixels = int((desc[:, 1].long().clamp(min=0) * desc[:, 2].long().clamp(min=0)).sum())
    stats = torch.empty((B, 8), dtype=torch.int32, device=buf.device)
    ws = mask_morphology_workspace(B, max(1, min(pixels, 2 ** 31 - 1)), buf.device)     # (a descriptor outside the limits is refused by the launcher, by image)
    check(lib().uia_mask_morphology(_stream(), B, _p(buf), buf.numel(), desc.data_ptr(), _p(ws), ws.numel(), _p(stats)), "uia_mask_morphology")
    return stats


# ---------------------------------------------------------------- DINOv2 UNet decoder (csrc/unet_conv.hip, unet_bn.hip, unet_resample.hip)
CONV3, CONVT_FWD, CONVT_BWD, CONV1 = 0, 1, 2, 3      # uia_conv_igemm / uia_conv_wgrad modes
BN_SLICES = 256                            # UIA_BN_SLICES


def _nhwc(t, name, dt=None):
    if t is None or t.dim() != 4 or not t.is_contiguous():
        raise UiaError(f"{name}: a contiguous NHWC [B, H, W, C] tensor is required")
    if dt is not None and t.dtype != dt:
        raise UiaError(f"{name}: dtype {t.dtype}, expected {dt}")
    return t


def conv_igemm(mode, x1, x2, w, n, bias=None, n1=None):
    """uia_conv_igemm.  CONV3: x1 [B,H,W,C1] (+ x2 [B,H,W,C2]) NHWC, w [n, 9·(C1+C2)] -> y [B,H,W,n], or (y1, y2) split at channel n1.
    CONVT_FWD: x1 [B,h,w,Cin], w [4·Cout, Cin], n = 4·Cout -> [B,2h,2w,Cout].  CONVT_BWD: x1 = dy [B,2h,2w,Cout], w [Cin, 4·Cout], n = Cin -> [B,h,w,Cin].
    CONV1: x1 [B,H,W,C1], w [n, C1] -> [B,H,W,n] (its data gradient: the same call on dy with the transposed weight)."""
    if mode not in (CONV3, CONVT_FWD, CONVT_BWD, CONV1):
        raise UiaError(f"conv_igemm: unknown mode {mode}")
    _nhwc(x1, "conv_igemm x1")
    dt = x1.dtype
    B, H, W, C1 = x1.shape
    C2 = 0
    if x2 is not None:
        _nhwc(x2, "conv_igemm x2", dt)
        if tuple(x2.shape[:3]) != (B, H, W):
            raise UiaError("conv_igemm: the two sources must share the pixel grid")
        C2 = x2.shape[3]
    if mode == CONVT_BWD:
        H, W = H // 2, W // 2
        if tuple(x1.shape[1:3]) != (2 * H, 2 * W):
            raise UiaError("conv_igemm: the transposed conv's gradient grid must be even")
    taps = {CONV3: 9, CONVT_FWD: 1, CONVT_BWD: 4, CONV1: 1}[mode]
    if w.dtype != dt or not w.is_contiguous() or tuple(w.shape) != (n, taps * (C1 + C2)):
        raise UiaError(f"conv_igemm: w must be contiguous {dt} [{n}, {taps * (C1 + C2)}], got {w.dtype} {tuple(w.shape)}")
    if bias is not None:
        nb = n // 4 if mode == CONVT_FWD else n
        if bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != nb:
            raise UiaError(f"conv_igemm: bias must be contiguous fp32 [{nb}]")
    n1 = n if n1 is None else int(n1)
    if mode == CONVT_FWD:
        y1 = torch.empty(B, 2 * H, 2 * W, n // 4, device=x1.device, dtype=dt)
    else:
        y1 = torch.empty(B, H, W, n1, device=x1.device, dtype=dt)
    y2 = torch.empty(B, H, W, n - n1, device=x1.device, dtype=dt) if n1 < n else None
    check(lib().uia_conv_igemm(_stream(), _code(dt), mode, B, H, W, C1, C2, _p(x1), _p(x2), n, n1, _p(w), _p(bias), _p(y1), _p(y2)), "uia_conv_igemm")
    return y1 if y2 is None else (y1, y2)


def conv_wgrad(mode, x1, x2, dy, n):
    """uia_conv_wgrad -> fp32 dW.  CONV3: dy [B,H,W,n] -> [n, 9·(C1+C2)].  CONVT_FWD: x1 [B,h,w,Cin], dy [B,2h,2w,n = Cout] -> [4·n, Cin].
    CONV1: dy [B,H,W,n] -> [n, C1]."""
    if mode not in (CONV3, CONVT_FWD, CONV1):
        raise UiaError(f"conv_wgrad: unknown mode {mode}")
    _nhwc(x1, "conv_wgrad x1")
    _nhwc(dy, "conv_wgrad dy", x1.dtype)
    B, H, W, C1 = x1.shape
    C2 = 0
    if x2 is not None:
        _nhwc(x2, "conv_wgrad x2", x1.dtype)
        C2 = x2.shape[3]
    want = (B, 2 * H, 2 * W, n) if mode == CONVT_FWD else (B, H, W, n)
    if tuple(dy.shape) != want:
        raise UiaError(f"conv_wgrad: dy {tuple(dy.shape)}, expected {want}")
    rows, cols = {CONV3: (n, 9 * (C1 + C2)), CONVT_FWD: (4 * n, C1), CONV1: (n, C1)}[mode]
    S = lib().uia_conv_wgrad_splits(mode, B, H, W, C1, C2, n)
    ws = torch.empty(S * rows * cols, device=x1.device, dtype=torch.float32) if S > 1 else None
    dw = torch.empty(rows, cols, device=x1.device, dtype=torch.float32)
    check(lib().uia_conv_wgrad(_stream(), _code(x1.dtype), mode, B, H, W, C1, C2, _p(x1), _p(x2), n, _p(dy), _p(ws), _p(dw)), "uia_conv_wgrad")
    return dw


def conv_igemm_form(mode, c1, c2, n, n1=None):
    """1 when uia_conv_igemm takes the matrix-core kernel for this shape (16-byte-aligned operands), 0 for the direct kernel.  No GPU needed."""
    return int(lib().uia_conv_igemm_form(int(mode), int(c1), int(c2), int(n), int(n if n1 is None else n1)))


def conv_wgrad_form(mode, c1, c2, n):
    """1 when uia_conv_wgrad takes the matrix-core kernel for this shape (16-byte-aligned operands), 0 for the direct kernel.  No GPU needed."""
    return int(lib().uia_conv_wgrad_form(int(mode), int(c1), int(c2), int(n)))


def colsum_ordered(y):
    """fp32 column sums of a contiguous [..., C] tensor in a fixed order (uia_colsum_ordered)."""
    if not y.is_contiguous():
        raise UiaError("colsum_ordered: contiguous rows required")
    C = y.shape[-1]
    M = y.numel() // C
    ws = torch.empty(BN_SLICES * C * 3, device=y.device, dtype=torch.float32)
    out = torch.empty(C, device=y.device, dtype=torch.float32)
    check(lib().uia_colsum_ordered(_stream(), _code(y.dtype), M, C, _p(y), _p(ws), _p(out)), "uia_colsum_ordered")
    return out


def _bn_fwd_args(name, y, gamma, beta, running_mean, running_var, num_batches_tracked, training):
    """What the three BatchNorm forwards share: the checks of y and the per-channel tensors, and the outputs.
    -> (M, C, out, mean, invstd, scale, shift, ws); mean / invstd / ws are None in eval mode."""
    _nhwc(y, f"{name} y")
    C = y.shape[3]
    M = y.numel() // C
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != C):
            raise UiaError(f"{name}: {nm} must be contiguous fp32 [{C}]")
    if num_batches_tracked is not None and num_batches_tracked.dtype != torch.int64:
        raise UiaError(f"{name}: num_batches_tracked must be int64")
    f = lambda: torch.empty(C, device=y.device, dtype=torch.float32)   # noqa: E731
    scale, shift = f(), f()
    mean, invstd, ws = (f(), f(), torch.empty(BN_SLICES * C * 3, device=y.device, dtype=torch.float32)) if training else (None, None, None)
    return M, C, torch.empty_like(y), mean, invstd, scale, shift, ws


def _bn_bwd_args(name, y, like, chans):
    """What the three BatchNorm backwards share: `like` ((tensor, its name), ...) must have y's layout, dtype and shape, `chans` must be
    per-channel fp32.  -> (M, C, dy, dgamma, dbeta, ws)"""
    _nhwc(y, f"{name} y")
    for t, nm in like:
        _nhwc(t, f"{name} {nm}", y.dtype)
    if any(t.shape != y.shape for t, _ in like):
        raise UiaError(f"{name}: {', '.join(nm for _, nm in like)} and y differ in shape")
    C = y.shape[3]
    for t, nm in chans:
        if t is None or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != C:
            raise UiaError(f"{name}: {nm} must be contiguous fp32 [{C}]")
    f = lambda: torch.empty(C, device=y.device, dtype=torch.float32)   # noqa: E731
    return y.numel() // C, C, torch.empty_like(y), f(), f(), torch.empty(BN_SLICES * C * 3, device=y.device, dtype=torch.float32)


def bn_fwd(y, gamma, beta, running_mean, running_var, num_batches_tracked, training, momentum=0.1, eps=1e-5, relu=True):
    """BatchNorm2d (+ ReLU) on NHWC y (uia_bn_fwd).  Returns (out, mean, invstd, scale, shift); mean / invstd are None in eval mode.
    Training updates running_mean / running_var / num_batches_tracked in place (any of them may be None: no update)."""
    M, C, out, mean, invstd, scale, shift, ws = _bn_fwd_args("bn_fwd", y, gamma, beta, running_mean, running_var, num_batches_tracked, training)
    check(lib().uia_bn_fwd(_stream(), _code(y.dtype), int(bool(training)), M, C, _p(y), _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                           _p(num_batches_tracked), float(momentum), float(eps), _p(ws), _p(mean), _p(invstd), _p(scale), _p(shift), int(bool(relu)), _p(out)),
          "uia_bn_fwd")
    return out, mean, invstd, scale, shift


def bn_relu_bwd(y, dout, scale, shift, mean, invstd, gamma):
    """Backward of train-mode BatchNorm2d + ReLU (uia_bn_relu_bwd): returns (dy, dgamma, dbeta)."""
    M, C, dy, dgamma, dbeta, ws = _bn_bwd_args("bn_relu_bwd", y, ((dout, "dout"),),
                                               ((scale, "scale"), (shift, "shift"), (mean, "mean"), (invstd, "invstd"), (gamma, "gamma")))
    check(lib().uia_bn_relu_bwd(_stream(), _code(y.dtype), M, C, _p(y), _p(dout), _p(scale), _p(shift), _p(mean), _p(invstd), _p(gamma), _p(ws),
                                _p(dgamma), _p(dbeta), _p(dy)), "uia_bn_relu_bwd")
    return dy, dgamma, dbeta


def _keep_mask(keep_mask, y, name):
    if keep_mask is None:
        return None
    if keep_mask.dtype != torch.uint8 or not keep_mask.is_contiguous() or keep_mask.shape != y.shape or keep_mask.device != y.device:
        raise UiaError(f"{name}: keep_mask must be contiguous uint8 of shape {tuple(y.shape)} on {y.device}, got {keep_mask.dtype} {tuple(keep_mask.shape)}")
    return keep_mask


def _drop_args(name, y, drop_p, keep_mask, training=True):
    drop_p = float(drop_p)
    if not 0.0 <= drop_p < 1.0:
        raise UiaError(f"{name}: drop_p={drop_p} outside [0, 1)")
    keep_mask = _keep_mask(keep_mask, y, name)
    if training and drop_p > 0.0 and keep_mask is None and y.numel() % 8:
        raise UiaError(f"{name}: the generated mask needs a multiple of 8 elements, got {y.numel()}")
    return drop_p, keep_mask


def bn_act_fwd(y, gamma, beta, running_mean, running_var, num_batches_tracked, training, momentum=0.1, eps=1e-5, slope=0.01, drop_p=0.0, seed=0,
               keep_mask=None):
    """BatchNorm2d + LeakyReLU(slope) + Dropout(drop_p) on NHWC y (uia_bn_act_fwd).  Returns (out, mean, invstd, scale, shift) as bn_fwd does.
    Dropout runs in training only: keep_mask (uint8, y's shape) when given, else the draw of ops.dropout for `seed`."""
    M, C, out, mean, invstd, scale, shift, ws = _bn_fwd_args("bn_act_fwd", y, gamma, beta, running_mean, running_var, num_batches_tracked, training)
    drop_p, keep_mask = _drop_args("bn_act_fwd", y, drop_p, keep_mask, training)
    check(lib().uia_bn_act_fwd(_stream(), _code(y.dtype), int(bool(training)), M, C, _p(y), _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                               _p(num_batches_tracked), float(momentum), float(eps), _p(ws), _p(mean), _p(invstd), _p(scale), _p(shift), float(slope), _p(out),
                               drop_p, int(seed) & 0xFFFFFFFFFFFFFFFF, _p(keep_mask)), "uia_bn_act_fwd")
    return out, mean, invstd, scale, shift


def bn_act_bwd(y, dout, scale, shift, mean, invstd, gamma, slope=0.01, drop_p=0.0, seed=0, keep_mask=None):
    """Backward of train-mode bn_act_fwd (uia_bn_act_bwd): returns (dy, dgamma, dbeta)."""
    M, C, dy, dgamma, dbeta, ws = _bn_bwd_args("bn_act_bwd", y, ((dout, "dout"),),
                                               ((scale, "scale"), (shift, "shift"), (mean, "mean"), (invstd, "invstd"), (gamma, "gamma")))
    drop_p, keep_mask = _drop_args("bn_act_bwd", y, drop_p, keep_mask)
    check(lib().uia_bn_act_bwd(_stream(), _code(y.dtype), M, C, _p(y), _p(dout), _p(scale), _p(shift), _p(mean), _p(invstd), _p(gamma), _p(ws),
                               _p(dgamma), _p(dbeta), _p(dy), float(slope), drop_p, int(seed) & 0xFFFFFFFFFFFFFFFF, _p(keep_mask)), "uia_bn_act_bwd")
    return dy, dgamma, dbeta


def maxpool2(x):
    """nn.MaxPool2d(2) on NHWC x [B,H,W,C] -> [B,H//2,W//2,C] (uia_maxpool2_fwd); a trailing odd row / column is ignored."""
    _nhwc(x, "maxpool2")
    B, H, W, C = x.shape
    if H < 2 or W < 2:
        raise UiaError(f"maxpool2: a grid of at least 2x2 is required, got {H}x{W}")
    y = torch.empty(B, H // 2, W // 2, C, device=x.device, dtype=x.dtype)
    check(lib().uia_maxpool2_fwd(_stream(), _code(x.dtype), B, H, W, C, _p(x), _p(y)), "uia_maxpool2_fwd")
    return y


def maxpool2_bwd(x, dy):
    """Backward of maxpool2 (uia_maxpool2_bwd): the argmax is recomputed from x; every element of dx [B,H,W,C] is written."""
    _nhwc(x, "maxpool2_bwd x")
    _nhwc(dy, "maxpool2_bwd dy", x.dtype)
    B, H, W, C = x.shape
    if H < 2 or W < 2:
        raise UiaError(f"maxpool2_bwd: a grid of at least 2x2 is required, got {H}x{W}")
    if tuple(dy.shape) != (B, H // 2, W // 2, C):
        raise UiaError(f"maxpool2_bwd: dy {tuple(dy.shape)}, expected {(B, H // 2, W // 2, C)}")
    dx = torch.empty_like(x)
    check(lib().uia_maxpool2_bwd(_stream(), _code(x.dtype), B, H, W, C, _p(x), _p(dy), _p(dx)), "uia_maxpool2_bwd")
    return dx


def upsample_ac(x, f, backward=False):
    """Bilinear upsample, align_corners=True, integer factor f, NHWC (uia_upsample_ac).  backward=True: x is dout [B,fH,fW,C] -> dx [B,H,W,C]."""
    _nhwc(x, "upsample_ac")
    B, H, W, C = x.shape
    f = int(f)
    if backward:
        if H % f or W % f:
            raise UiaError(f"upsample_ac: gradient grid {H}x{W} is not a multiple of {f}")
        H, W = H // f, W // f
        out = torch.empty(B, H, W, C, device=x.device, dtype=x.dtype)
    else:
        out = torch.empty(B, H * f, W * f, C, device=x.device, dtype=x.dtype)
    check(lib().uia_upsample_ac(_stream(), _code(x.dtype), int(bool(backward)), B, H, W, C, f, _p(x), _p(out)), "uia_upsample_ac")
    return out


def resize_aa(x, size):
    """Antialiased bicubic resize (align_corners=False) of NHWC x [B,Hi,Wi,C] to NCHW fp32 [B,C,Ho,Wo] (uia_resize_aa)."""
    _nhwc(x, "resize_aa")
    B, Hi, Wi, C = x.shape
    Ho, Wo = size
    tmp = torch.empty(B * C * Hi * Wo, device=x.device, dtype=torch.float32)
    out = torch.empty(B, C, Ho, Wo, device=x.device, dtype=torch.float32)
    check(lib().uia_resize_aa(_stream(), _code(x.dtype), 0, B, C, Hi, Wi, Ho, Wo, _p(x), _p(tmp), _p(out), None, None), "uia_resize_aa")
    return out


def resize_aa_bwd(dout, in_hw, dtype):
    """Backward of resize_aa: dout fp32 NCHW [B,C,Ho,Wo] -> dx NHWC [B,Hi,Wi,C] in dtype."""
    if dout.dim() != 4 or dout.dtype != torch.float32 or not dout.is_contiguous():
        raise UiaError("resize_aa_bwd: dout must be contiguous fp32 [B, C, Ho, Wo]")
    B, C, Ho, Wo = dout.shape
    Hi, Wi = in_hw
    tmp = torch.empty(B * C * Hi * Wo, device=dout.device, dtype=torch.float32)
    dx = torch.empty(B, Hi, Wi, C, device=dout.device, dtype=dtype)
    check(lib().uia_resize_aa(_stream(), _code(dtype), 1, B, C, Hi, Wi, Ho, Wo, None, _p(tmp), None, _p(dout), _p(dx)), "uia_resize_aa")
    return dx


# ---------------------------------------------------------------- ResNet baseline (csrc/unet_conv.hip, unet_pool.hip, unet_bn.hip)
def _strided_ks(name, k, s):
    k, s = int(k), int(s)
    if k not in (1, 3, 7) or s not in (1, 2):
        raise UiaError(f"{name}: kernel size {k} / stride {s} not built (k in 1, 3, 7; s in 1, 2)")
    return k, s


def strided_out_hw(h, w, s):
    """The output grid of Conv2d(k, stride s, padding k//2) for odd k, and of MaxPool2d(3, 2, 1) at s = 2."""
    return (h - 1) // s + 1, (w - 1) // s + 1


def conv_strided(x, w, n, k, s):
    """uia_conv_strided forward: Conv2d(k, stride s, padding k//2, bias=False) of NHWC x [B,H,W,C] with w [n, k·k·C] -> [B,Ho,Wo,n]."""
    k, s = _strided_ks("conv_strided", k, s)
    _nhwc(x, "conv_strided x")
    B, H, W, C = x.shape
    if w.dtype != x.dtype or not w.is_contiguous() or tuple(w.shape) != (n, k * k * C):
        raise UiaError(f"conv_strided: w must be contiguous {x.dtype} [{n}, {k * k * C}], got {w.dtype} {tuple(w.shape)}")
    Ho, Wo = strided_out_hw(H, W, s)
    y = torch.empty(B, Ho, Wo, n, device=x.device, dtype=x.dtype)
    check(lib().uia_conv_strided(_stream(), _code(x.dtype), 0, B, H, W, C, k, s, _p(x), n, _p(w), _p(y)), "uia_conv_strided")
    return y


def conv_strided_dgrad(dy, w, in_hw, c, k, s):
    """uia_conv_strided data gradient: dy [B,Ho,Wo,n], w [c, k·k·n] (column (ky·k + kx)·n + o) -> dx [B,H,W,c] for the conv's input grid in_hw."""
    k, s = _strided_ks("conv_strided_dgrad", k, s)
    _nhwc(dy, "conv_strided_dgrad dy")
    B, Ho, Wo, n = dy.shape
    H, W = in_hw
    if (Ho, Wo) != strided_out_hw(H, W, s):
        raise UiaError(f"conv_strided_dgrad: dy grid {Ho}x{Wo} is not the stride-{s} output of {H}x{W}")
    if w.dtype != dy.dtype or not w.is_contiguous() or tuple(w.shape) != (c, k * k * n):
        raise UiaError(f"conv_strided_dgrad: w must be contiguous {dy.dtype} [{c}, {k * k * n}], got {w.dtype} {tuple(w.shape)}")
    dx = torch.empty(B, H, W, c, device=dy.device, dtype=dy.dtype)
    check(lib().uia_conv_strided(_stream(), _code(dy.dtype), 1, B, H, W, c, k, s, _p(dy), n, _p(w), _p(dx)), "uia_conv_strided")
    return dx


def conv_strided_wgrad(x, dy, k, s):
    """uia_conv_strided_wgrad -> fp32 dW [n, k·k·C] from x [B,H,W,C] and dy [B,Ho,Wo,n]."""
    k, s = _strided_ks("conv_strided_wgrad", k, s)
    _nhwc(x, "conv_strided_wgrad x")
    _nhwc(dy, "conv_strided_wgrad dy", x.dtype)
    B, H, W, C = x.shape
    n = dy.shape[3]
    if tuple(dy.shape[:3]) != (B, *strided_out_hw(H, W, s)):
        raise UiaError(f"conv_strided_wgrad: dy {tuple(dy.shape)}, expected {(B, *strided_out_hw(H, W, s), n)}")
    cols = k * k * C
    S = lib().uia_conv_strided_wgrad_splits(B, H, W, C, k, s, n)
    ws = torch.empty(S * n * cols, device=x.device, dtype=torch.float32) if S > 1 else None
    dw = torch.empty(n, cols, device=x.device, dtype=torch.float32)
    check(lib().uia_conv_strided_wgrad(_stream(), _code(x.dtype), B, H, W, C, k, s, _p(x), n, _p(dy), _p(ws), _p(dw)), "uia_conv_strided_wgrad")
    return dw


def conv_strided_form(dgrad, c, n, k, s):
    """1 when uia_conv_strided takes the matrix-core kernel for this shape (16-byte-aligned operands), 0 for the direct kernel.  No GPU needed."""
    return int(lib().uia_conv_strided_form(int(dgrad), int(c), int(n), int(k), int(s)))


def conv_strided_wgrad_form(c, n, k, s):
    """1 when uia_conv_strided_wgrad takes the matrix-core kernel for this shape (16-byte-aligned operands), 0 for the direct kernel.  No GPU needed."""
    return int(lib().uia_conv_strided_wgrad_form(int(c), int(n), int(k), int(s)))


def maxpool3s2(x):
    """nn.MaxPool2d(3, 2, 1) on NHWC x [B,H,W,C] -> [B,(H-1)//2+1,(W-1)//2+1,C] (uia_maxpool3s2_fwd); the padding is -inf."""
    _nhwc(x, "maxpool3s2")
    B, H, W, C = x.shape
    y = torch.empty(B, *strided_out_hw(H, W, 2), C, device=x.device, dtype=x.dtype)
    check(lib().uia_maxpool3s2_fwd(_stream(), _code(x.dtype), B, H, W, C, _p(x), _p(y)), "uia_maxpool3s2_fwd")
    return y


def maxpool3s2_bwd(x, dy):
    """Backward of maxpool3s2 (uia_maxpool3s2_bwd): the argmax is recomputed from x; every element of dx [B,H,W,C] is written."""
    _nhwc(x, "maxpool3s2_bwd x")
    _nhwc(dy, "maxpool3s2_bwd dy", x.dtype)
    B, H, W, C = x.shape
    want = (B, *strided_out_hw(H, W, 2), C)
    if tuple(dy.shape) != want:
        raise UiaError(f"maxpool3s2_bwd: dy {tuple(dy.shape)}, expected {want}")
    dx = torch.empty_like(x)
    check(lib().uia_maxpool3s2_bwd(_stream(), _code(x.dtype), B, H, W, C, _p(x), _p(dy), _p(dx)), "uia_maxpool3s2_bwd")
    return dx


def bn_add_relu_fwd(y, r, gamma, beta, running_mean, running_var, num_batches_tracked, training, momentum=0.1, eps=1e-5):
    """relu(BatchNorm2d(y) + r) on NHWC y, r (uia_bn_add_relu_fwd; r may be None).  Returns (out, mean, invstd, scale, shift) as bn_fwd does."""
    _nhwc(y, "bn_add_relu_fwd y")
    if r is not None:
        _nhwc(r, "bn_add_relu_fwd r", y.dtype)
        if r.shape != y.shape:
            raise UiaError("bn_add_relu_fwd: r and y differ in shape")
    M, C, out, mean, invstd, scale, shift, ws = _bn_fwd_args("bn_add_relu_fwd", y, gamma, beta, running_mean, running_var, num_batches_tracked, training)
    check(lib().uia_bn_add_relu_fwd(_stream(), _code(y.dtype), int(bool(training)), M, C, _p(y), _p(r), _p(gamma), _p(beta), _p(running_mean),
                                    _p(running_var), _p(num_batches_tracked), float(momentum), float(eps), _p(ws), _p(mean), _p(invstd), _p(scale),
                                    _p(shift), _p(out)), "uia_bn_add_relu_fwd")
    return out, mean, invstd, scale, shift


def bn_add_relu_bwd(y, out, dout, mean, invstd, gamma, want_dr=True):
    """Backward of train-mode bn_add_relu_fwd (uia_bn_add_relu_bwd): returns (dy, dr, dgamma, dbeta); dr is None without want_dr."""
    M, C, dy, dgamma, dbeta, ws = _bn_bwd_args("bn_add_relu_bwd", y, ((out, "out"), (dout, "dout")), ((mean, "mean"), (invstd, "invstd"), (gamma, "gamma")))
    dr = torch.empty_like(y) if want_dr else None
    check(lib().uia_bn_add_relu_bwd(_stream(), _code(y.dtype), M, C, _p(y), _p(out), _p(dout), _p(mean), _p(invstd), _p(gamma), _p(ws), _p(dgamma),
                                    _p(dbeta), _p(dy), _p(dr)), "uia_bn_add_relu_bwd")
    return dy, dr, dgamma, dbeta


def avgpool(x):
    """Global average pool of NHWC x [B,H,W,C] -> fp32 [B,C] (uia_avgpool_fwd)."""
    _nhwc(x, "avgpool")
    B, H, W, C = x.shape
    out = torch.empty(B, C, device=x.device, dtype=torch.float32)
    check(lib().uia_avgpool_fwd(_stream(), _code(x.dtype), B, H, W, C, _p(x), _p(out)), "uia_avgpool_fwd")
    return out


def avgpool_bwd(dout, hw, dtype):
    """Backward of avgpool: fp32 dout [B,C] -> dx [B,H,W,C] in dtype, dout/(H·W) at every pixel (uia_avgpool_bwd)."""
    if dout.dim() != 2 or dout.dtype != torch.float32 or not dout.is_contiguous():
        raise UiaError("avgpool_bwd: dout must be contiguous fp32 [B, C]")
    B, C = dout.shape
    H, W = hw
    dx = torch.empty(B, H, W, C, device=dout.device, dtype=dtype)
    check(lib().uia_avgpool_bwd(_stream(), _code(dtype), B, H, W, C, _p(dout), _p(dx)), "uia_avgpool_bwd")
    return dx


def nchw_to_nhwc(x, cout, rep, dtype):
    """uia_nchw_to_nhwc: fp32 NCHW x [B,Cin,H,W] -> NHWC [B,H,W,cout] of dtype; channels c < rep filled (a one-channel x repeated), the rest zero."""
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise UiaError("nchw_to_nhwc: x must be contiguous fp32 [B, C, H, W]")
    B, Cin, H, W = x.shape
    if not (0 <= rep <= cout and (rep <= Cin or Cin == 1)):
        raise UiaError(f"nchw_to_nhwc: {rep} filled channels from {Cin} sources into {cout}")
    out = torch.empty(B, H, W, cout, device=x.device, dtype=dtype)
    check(lib().uia_nchw_to_nhwc(_stream(), _code(dtype), B, Cin, H, W, int(cout), int(rep), _p(x), _p(out)), "uia_nchw_to_nhwc")
    return out


def add2(a, b):
    """a + b element-wise (uia_add2): the sum of a residual block's two input gradients."""
    if a.shape != b.shape or a.dtype != b.dtype or not a.is_contiguous() or not b.is_contiguous():
        raise UiaError("add2: two contiguous tensors of one shape and dtype are required")
    out = torch.empty_like(a)
    check(lib().uia_add2(_stream(), _code(a.dtype), a.numel(), _p(a), _p(b), _p(out)), "uia_add2")
    return out
