"""-m gpu: uia_seg_predict_native_ens (csrc/seg_native_ens.hip) — masks, overlays, probability and spread maps, statistics and sums of a ragged batch from
K members' S x S logits, one launch.

Reference: float64 on the CPU — every member's planes flipped back, F.interpolate(size=(H, W), mode="bilinear", align_corners=False), p_k = sigmoid(u_1 -
u_0), P = mean, spread = max - min.
Margins: m_d = (12 S + 16) 2^-24 max|logits of that image over all members| is tests/test_seg_native_gpu.py's margin on a logit difference; m_P = m_d / 4 +
2^-20 on a probability (the sigmoid's slope is at most 1/4; 2^-20 covers expf, the division and the K-term sum).
  mask: a pixel with |P_ref - threshold| <= m_P may differ, every other pixel must agree;
  probability byte: within 1 of the reference byte everywhere, equal wherever 255 P_ref + 0.5 lies more than 255 m_P from an integer;
  spread byte: the same with 2 m_P.
How many pixels the margins excuse is capped by assertions on the reference alone, before anything is compared: per image at most 4 + 0.001 H W pixels
inside the mask margin; over the batch at most 6 % of the probability bytes and 12 % of the spread bytes excluded from exact equality.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_seg_native_gpu import EMPTY, GUARD, SENTINEL, box_of, dev, sizes_for  # noqa: E402

pytestmark = pytest.mark.gpu
MEMBERS = [(1, [0]), (3, [0, 1, 2]), (4, [0, 1, 2, 3]), (16, [k % 4 for k in range(16)])]
THRESHOLDS = [0.5, 0.35]
KINDS = ("mask", "overlay", "prob", "spread")


class Batch:
    """The ragged batch of tests/test_seg_native_gpu.py laid out the same awkward way — image 0 one byte into the source buffer, every output range at an odd
    offset behind a gap of sentinel bytes, guard bytes at both ends — with a probability and a spread range per image; `without` lists (image, kind)
    pairs that get -1 instead."""

    def __init__(self, sizes, without=(), seed=0, with_src=True):
        rng = np.random.default_rng(seed)
        self.sizes, self.B = list(sizes), len(sizes)
        at, rows = 1, []
        for H, W in self.sizes:
            rows.append(at)
            at += H * W
        self.src_host = rng.integers(0, 256, size=at, dtype=np.uint8)
        self.src = torch.from_numpy(self.src_host).to(dev()) if with_src else None
        at, self.ranges, desc = GUARD + 1, [], []
        for b, (H, W) in enumerate(self.sizes):
            offs = {}
            for kind, planes, gap in (("mask", 1, 3), ("overlay", 3, 5), ("prob", 1, 7), ("spread", 1, 1)):
                offs[kind] = -1
                if (b, kind) in without or (kind == "overlay" and not with_src):
                    continue
                offs[kind], at = at, at + planes * H * W + gap
                at += (at + 1) % 2                               # the next range starts odd
            desc.append([rows[b] if with_src else -1, H, W, offs["mask"], offs["overlay"], offs["prob"], offs["spread"], 0])
            self.ranges.append(offs)
        self.total = at + GUARD
        self.desc = torch.tensor(desc, dtype=torch.int32)
        self.out = torch.full((self.total,), SENTINEL, dtype=torch.uint8, device=dev())
        self.stats = torch.full((self.B, 8), 77, dtype=torch.int32, device=dev())
        self.sums = torch.full((self.B, 2), 77, dtype=torch.int64, device=dev())

    def run(self, logits, flips, threshold=0.5):
        """-> (the output buffer's bytes, stats, sums) on the host."""
        from uia_hip import ops
        ops.seg_predict_native_ens(logits, flips, self.src, self.desc, self.out, threshold=threshold, stats=self.stats, sums=self.sums)
        torch.cuda.synchronize()
        return self.out.cpu().numpy().copy(), self.stats.cpu().numpy().copy(), self.sums.cpu().numpy().copy()

    def plane(self, flat, b, kind):
        H, W = self.sizes[b]
        off = self.ranges[b][kind]
        return flat[off:off + 3 * H * W].reshape(H, W, 3) if kind == "overlay" else flat[off:off + H * W].reshape(H, W)

    def gray(self, b):
        H, W = self.sizes[b]
        off = int(self.desc[b, 0])
        return self.src_host[off:off + H * W].reshape(H, W)

    def outside_is_intact(self, flat):
        covered = np.zeros(self.total, dtype=bool)
        for (H, W), offs in zip(self.sizes, self.ranges):
            for kind in KINDS:
                if offs[kind] >= 0:
                    covered[offs[kind]:offs[kind] + (3 if kind == "overlay" else 1) * H * W] = True
        return bool((flat[~covered] == SENTINEL).all())


def unflip(planes, f):
    """L'[y][x] = L[fy ? S-1-y : y][fx ? S-1-x : x] of [..., S, S] planes (a flip is its own inverse)."""
    dims = [d for d, bit in ((-1, 1), (-2, 2)) if f & bit]
    return torch.flip(planes, dims) if dims else planes


def member_probabilities(logits, flips, b, H, W):
    """float64 [K, H, W]: p_k of image b at its own size."""
    rows = []
    for k, f in enumerate(flips):
        u = F.interpolate(unflip(logits[k, b], f)[None].double(), size=(H, W), mode="bilinear", align_corners=False)[0]
        rows.append(torch.sigmoid(u[1] - u[0]))
    return torch.stack(rows).numpy()


def off_integer(v, margin):
    """True where the float64 v lies more than `margin` from the nearest integer boundary of floor(v): the byte floor(v) is then certain."""
    return np.abs(v - np.round(v)) > margin


@functools.lru_cache(maxsize=None)
def reference(S, K):
    """-> (logits, flips, per image (P, spread, m_d, m_P)) with the byte caps asserted on the reference alone."""
    flips = dict(MEMBERS)[K]
    torch.manual_seed(100 + K)
    logits = 3 * torch.randn(K, 8, 2, S, S)
    out, pixels, loose_q, loose_r = [], 0, 0, 0
    for b, (H, W) in enumerate(sizes_for(S)):
        p = member_probabilities(logits, flips, b, H, W)
        P, spread = p.mean(axis=0), p.max(axis=0) - p.min(axis=0)
        m_d = (12 * S + 16) * 2.0 ** -24 * float(logits[:, b].abs().max())
        m_P = m_d / 4 + 2.0 ** -20
        pixels += H * W
        loose_q += int((~off_integer(255 * P + 0.5, 255 * m_P)).sum())
        loose_r += int((~off_integer(255 * spread + 0.5, 255 * 2 * m_P)).sum())
        out.append((P, spread, m_d, m_P))
    print(f"S={S} K={K}: {loose_q / pixels:.4f} of the probability bytes and {loose_r / pixels:.4f} of the spread bytes are excluded from exact equality")
    assert loose_q <= 0.06 * pixels and loose_r <= 0.12 * pixels, (S, K, loose_q, loose_r, pixels)
    return logits, flips, out


@functools.lru_cache(maxsize=None)
def case(S, K, threshold):
    """The issue's batch at (S, K, threshold), run twice: (batch, reference rows, first (bytes, stats, sums), second)."""
    logits, flips, ref = reference(S, K)
    for b, ((H, W), (P, _, _, m_P)) in enumerate(zip(sizes_for(S), ref)):
        inside = int((np.abs(P - threshold) <= m_P).sum())
        print(f"S={S} K={K} t={threshold} image {b} {H}x{W}: m_P {m_P:.3e}, {inside} of {H * W} pixels inside the mask margin")
        assert inside <= 4 + 0.001 * H * W, (S, K, threshold, b, inside)
    batch = Batch(sizes_for(S), without=((2, "overlay"),), seed=S + K)
    lg = logits.to(dev())
    first = batch.run(lg, flips, threshold)
    second = batch.run(lg, flips, threshold)
    return batch, ref, first, second


def cases(fn):
    return pytest.mark.parametrize("threshold", THRESHOLDS)(pytest.mark.parametrize("K", [k for k, _ in MEMBERS])(pytest.mark.parametrize("S", [8, 32])(fn)))


# ------------------------------------------------------------------------------------------------ 1. against float64
@cases
def test_masks_and_maps_agree_with_float64_outside_the_margins(S, K, threshold):
    batch, ref, (flat, _, _), _ = case(S, K, threshold)
    assert int(batch.desc[0, 0]) == 1 and batch.ranges[2]["overlay"] == -1
    assert all(off % 2 == 1 for offs in batch.ranges for off in offs.values() if off >= 0)
    for b, ((H, W), (P, spread, _, m_P)) in enumerate(zip(batch.sizes, ref)):
        mask, q, r = (batch.plane(flat, b, kind) for kind in ("mask", "prob", "spread"))
        assert set(np.unique(mask)) <= {0, 255}, (S, K, b)
        sure = np.abs(P - threshold) > m_P
        wrong = int(((mask > 0) != (P > threshold))[sure].sum())
        for name, got, want, margin in (("probability", q, 255 * P + 0.5, 255 * m_P), ("spread", r, 255 * spread + 0.5, 255 * 2 * m_P)):
            byte = np.floor(want).astype(np.int64)
            diff = np.abs(got.astype(np.int64) - byte)
            exact = off_integer(want, margin)
            print(f"S={S} K={K} t={threshold} image {b} {H}x{W} {name}: worst byte difference {int(diff.max())}, {int((diff[exact] != 0).sum())} differ where none may")
            assert int(diff.max()) <= 1, (S, K, b, name)
            assert not diff[exact].any(), (S, K, b, name)
        print(f"S={S} K={K} t={threshold} image {b} {H}x{W}: {wrong} mask pixels differ outside the margin")
        assert wrong == 0, (S, K, threshold, b, wrong)
        if K == 1:
            assert not r.any(), (S, b)


# ------------------------------------------------------------------------------------------------ 2. exact properties of the kernel's own bytes
@cases
def test_stats_sums_and_overlays_follow_from_the_returned_bytes(S, K, threshold):
    batch, _, (flat, stats, sums), _ = case(S, K, threshold)
    for b in range(batch.B):
        mask, q, r = (batch.plane(flat, b, kind) for kind in ("mask", "prob", "spread"))
        assert stats[b].tolist() == box_of(mask), (S, K, b)
        assert sums[b].tolist() == [int(q[mask == 255].astype(np.int64).sum()), int(r.astype(np.int64).sum())], (S, K, b)
        if batch.ranges[b]["overlay"] >= 0:
            g = batch.gray(b)
            assert np.array_equal(batch.plane(flat, b, "overlay"), np.stack([g, np.maximum(g, mask), g], axis=-1)), (S, K, b)


@cases
def test_nothing_is_written_outside_the_ranges_and_two_calls_agree(S, K, threshold):
    batch, _, (flat, stats, sums), (flat2, stats2, sums2) = case(S, K, threshold)
    assert batch.outside_is_intact(flat)
    assert np.array_equal(flat, flat2) and np.array_equal(stats, stats2) and np.array_equal(sums, sums2)
    assert not (stats[:, 5:] != 0).any()


@pytest.mark.parametrize("S", [8, 32])
def test_flipped_copies_of_one_tensor_give_the_bytes_of_unflipped_copies(S):
    torch.manual_seed(7)
    base = 3 * torch.randn(8, 2, S, S)
    flips = [0, 1, 2, 3, 3, 2, 1]
    flipped = torch.stack([unflip(base, f) for f in flips]).contiguous()
    copies = torch.stack([base] * len(flips)).contiguous()
    a, b = Batch(sizes_for(S), seed=1), Batch(sizes_for(S), seed=1)
    fa, sa, qa = a.run(flipped.to(dev()), flips, 0.35)
    fb, sb, qb = b.run(copies.to(dev()), [0] * len(flips), 0.35)
    assert np.array_equal(fa, fb) and np.array_equal(sa, sb) and np.array_equal(qa, qb)
    assert not flipped[1].equal(base) and sa[:, 0].max() > 0
    for i in range(a.B):
        assert not a.plane(fa, i, "spread").any(), i
    assert not qa[:, 1].any()


@pytest.mark.parametrize("S", [8, 32])
def test_one_member_at_one_half_is_seg_predict_native_up_to_the_margin(S):
    from uia_hip import ops
    torch.manual_seed(0)
    logits = 3 * torch.randn(8, 2, S, S)
    sizes = sizes_for(S)
    batch = Batch(sizes, seed=2)
    flat, stats, _ = batch.run(logits[None].contiguous().to(dev()), [0], 0.5)
    at, rows = 0, []
    for H, W in sizes:
        rows.append([-1, H, W, at, -1, 0, 0, 0])
        at += H * W
    plain = torch.zeros(at, dtype=torch.uint8, device=dev())
    ops.seg_predict_native(logits.to(dev()), None, torch.tensor(rows, dtype=torch.int32), plain)
    plain = plain.cpu().numpy()
    for b, (H, W) in enumerate(sizes):
        u = F.interpolate(logits[b:b + 1].double(), size=(H, W), mode="bilinear", align_corners=False)[0]
        d = (u[1] - u[0]).numpy()
        m_d = (12 * S + 16) * 2.0 ** -24 * float(logits[b].abs().max())
        differ = batch.plane(flat, b, "mask") != plain[rows[b][3]:rows[b][3] + H * W].reshape(H, W)
        print(f"S={S} image {b} {H}x{W}: {int(differ.sum())} pixels differ from seg_predict_native")
        assert (np.abs(d[differ]) <= m_d).all(), (S, b)


# ------------------------------------------------------------------------------------------------ 3. optional ranges, sums = NULL
def raw_call(K, B, S, logits, flips, threshold, src, src_bytes, desc, out, out_bytes, ws, ws_bytes, stats, sums):
    from uia_hip import _lib
    lib = _lib.lib()
    d = np.ascontiguousarray(desc, dtype=np.int32)
    rc = lib.uia_seg_predict_native_ens(torch.cuda.current_stream().cuda_stream, K, B, S, logits, flips, threshold, src, src_bytes, d.ctypes.data, out, out_bytes,
                                        ws, ws_bytes, stats, sums)
    torch.cuda.synchronize()                                     # (the pageable descriptor has been read before it goes away)
    return rc, lib.uia_last_error().decode()


def test_each_optional_range_absent_in_turn_and_no_sums():
    from uia_hip import ops
    S, sizes, flips = 8, [(9, 11), (8, 8), (20, 3)], [0, 3]
    torch.manual_seed(5)
    logits = (3 * torch.randn(2, 3, 2, S, S)).to(dev())
    full = Batch(sizes, seed=6)
    flat, stats, sums = full.run(logits, flips, 0.35)
    for kind in ("overlay", "prob", "spread"):
        part = Batch(sizes, without=tuple((b, kind) for b in range(3)), seed=6)
        got, st, sm = part.run(logits, flips, 0.35)
        assert (part.desc[:, 4 + KINDS.index(kind) - 1] == -1).all()
        for b in range(3):
            for other in KINDS:
                if other != kind:
                    assert np.array_equal(part.plane(got, b, other), full.plane(flat, b, other)), (kind, other, b)
        assert np.array_equal(st, stats) and np.array_equal(sm, sums) and part.outside_is_intact(got), kind      # the sums do not need the maps
    none = Batch(sizes, seed=6, with_src=False)
    got, st, sm = none.run(logits, flips, 0.35)
    assert none.src is None and (none.desc[:, 0] == -1).all() and (none.desc[:, 4] == -1).all()
    assert np.array_equal(st, stats) and np.array_equal(sm, sums) and none.outside_is_intact(got)
    # sums = NULL at the C boundary: everything else as before, the tensor handed in earlier untouched
    again = Batch(sizes, seed=6)
    ws = ops.seg_native_ens_workspace(3, dev())
    rc, err = raw_call(2, 3, S, logits.data_ptr(), 0b1100, 0.35, again.src.data_ptr(), again.src.numel(), again.desc.numpy(), again.out.data_ptr(), again.total,
                       ws.data_ptr(), ws.numel(), again.stats.data_ptr(), None)
    assert rc == 0, err
    assert np.array_equal(again.out.cpu().numpy(), flat) and np.array_equal(again.stats.cpu().numpy(), stats) and bool((again.sums == 77).all())


# ------------------------------------------------------------------------------------------------ 4. NaN and infinities
def test_nan_and_infinity_rules():
    """A pixel where any member's z is NaN: mask 0, q 0, r 255.  Infinite logits follow IEEE: z = +inf is p = 1, z = -inf is p = 0, inf - inf is NaN.  At
    H = W = S no tap but the pixel's own enters, so planted values stay where they are; elsewhere whole planes are planted."""
    S, nan, inf = 8, float("nan"), float("inf")
    torch.manual_seed(4)
    logits = torch.randn(2, 7, 2, S, S)
    logits[1, 0, 1] = nan                                        # image 0, upscaled: one member's class 1 all NaN
    logits[0, 1, 0, 2, 3] = nan                                  # image 1, identity size: one pixel of member 0, another of member 1
    logits[1, 1, 1, 6, 6] = nan
    logits[:, 2, 1] = inf                                        # image 2: z = +inf in both members
    logits[:, 3, 1] = -inf                                       # image 3: z = -inf in both
    logits[0, 4, 1], logits[1, 4, 1] = inf, -inf                 # image 4: p = 1 and p = 0
    logits[0, 5] = inf                                           # image 5: inf - inf in member 0
    logits[1, 6, 0] = inf                                        # image 6: member 1 says 0 for certain, member 0 is ordinary
    sizes = [(11, 13), (8, 8), (12, 9), (5, 7), (20, 20), (3, 3), (8, 8)]
    batch = Batch(sizes, seed=5)
    flat, stats, sums = batch.run(logits.to(dev()), [0, 0], 0.5)
    mask, q, r = ([batch.plane(flat, b, kind) for b in range(7)] for kind in ("mask", "prob", "spread"))
    for b in (0, 5):
        assert not mask[b].any() and not q[b].any() and (r[b] == 255).all() and stats[b].tolist() == EMPTY, b
        assert sums[b].tolist() == [0, 255 * sizes[b][0] * sizes[b][1]], b
    planted = np.zeros((8, 8), dtype=bool)
    planted[2, 3] = planted[6, 6] = True
    assert (mask[1][planted] == 0).all() and (q[1][planted] == 0).all() and (r[1][planted] == 255).all()
    z = (logits[:, 1, 1] - logits[:, 1, 0]).double()
    p = torch.sigmoid(z).numpy()
    want = np.floor(255 * p.mean(axis=0) + 0.5)
    assert (np.abs(q[1].astype(np.int64) - want)[~planted] <= 1).all() and (r[1][~planted] < 255).all()
    assert (mask[2] == 255).all() and (q[2] == 255).all() and not r[2].any() and stats[2].tolist() == [108, 0, 0, 11, 8, 0, 0, 0]
    assert sums[2].tolist() == [255 * 108, 0]
    assert not mask[3].any() and not q[3].any() and not r[3].any() and sums[3].tolist() == [0, 0]
    assert not mask[4].any() and (q[4] == 128).all() and (r[4] == 255).all()          # P = 0.5 exactly is not above the threshold
    half = np.floor(255 * torch.sigmoid((logits[0, 6, 1] - logits[0, 6, 0]).double()).numpy() / 2 + 0.5)
    assert not mask[6].any() and (np.abs(q[6].astype(np.int64) - half) <= 1).all()
    assert batch.outside_is_intact(flat)


# ------------------------------------------------------------------------------------------------ 5. the 64-bit sum
def test_a_sum_beyond_32_bits():
    """4200 x 4096 pixels of probability byte 255: 255 * 17 203 200 > 2^32.  A row of 4096 pixels is also wider than one workgroup's run."""
    from uia_hip import ops
    S, H, W = 8, 4200, 4096
    logits = torch.empty(1, 1, 2, S, S, device=dev())
    logits[:, :, 0], logits[:, :, 1] = -20.0, 20.0
    out = torch.full((2 * H * W + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=dev())
    desc = torch.tensor([[-1, H, W, GUARD, -1, GUARD + H * W, -1, 0]], dtype=torch.int32)
    stats, sums = ops.seg_predict_native_ens(logits, [0], None, desc, out)
    torch.cuda.synchronize()
    assert bool((out[GUARD:GUARD + 2 * H * W] == 255).all()) and bool((out[:GUARD] == SENTINEL).all()) and bool((out[GUARD + 2 * H * W:] == SENTINEL).all())
    assert stats.cpu().tolist() == [[H * W, 0, 0, H - 1, W - 1, 0, 0, 0]]
    assert sums.cpu().tolist() == [[255 * H * W, 0]] and 255 * H * W > 2 ** 32


def test_tiles_limited_by_the_width_and_by_S():
    """The rows of a run: 8 in the cases above; 1 with column pieces for a 5 000 wide image; 4 at S = 1024 (the blended rows fit 32 KiB).  The S = 1024
    case is exact in fp32 and in float64 alike up to the sigmoid — integer logits, a 2x downscale, weights of 1/2 — so only its bytes carry a margin."""
    torch.manual_seed(2)
    logits = 3 * torch.randn(2, 2, 2, 8, 8)
    sizes, flips = [(9, 5000), (2, 16384)], [0, 3]
    batch = Batch(sizes, seed=2)
    flat, stats, sums = batch.run(logits.to(dev()), flips, 0.5)
    for b, (H, W) in enumerate(sizes):
        p = member_probabilities(logits, flips, b, H, W)
        P, m_P = p.mean(axis=0), (12 * 8 + 16) * 2.0 ** -24 * float(logits[:, b].abs().max()) / 4 + 2.0 ** -20
        mask, q, r = (batch.plane(flat, b, kind) for kind in ("mask", "prob", "spread"))
        assert not ((mask > 0) != (P > 0.5))[np.abs(P - 0.5) > m_P].any(), b
        assert (np.abs(q.astype(np.int64) - np.floor(255 * P + 0.5)) <= 1).all() and (np.abs(r.astype(np.int64) - np.floor(255 * (p.max(axis=0) - p.min(axis=0)) + 0.5)) <= 1).all()
        assert stats[b].tolist() == box_of(mask) and sums[b].tolist() == [int(q[mask == 255].astype(np.int64).sum()), int(r.astype(np.int64).sum())]
        g = batch.gray(b)
        assert np.array_equal(batch.plane(flat, b, "overlay"), np.stack([g, np.maximum(g, mask), g], axis=-1))
    assert batch.outside_is_intact(flat)

    big = torch.randint(-8, 9, (1, 1, 2, 1024, 1024), generator=torch.Generator().manual_seed(3)).float()
    u = F.interpolate(big[0].double(), size=(512, 512), mode="bilinear", align_corners=False)[0]
    P = torch.sigmoid(u[1] - u[0]).numpy()
    one = Batch([(512, 512)], seed=4)
    flat, stats, _ = one.run(big.to(dev()), [0], 0.5)
    assert np.array_equal(one.plane(flat, 0, "mask") > 0, P > 0.5)
    assert (np.abs(one.plane(flat, 0, "prob").astype(np.int64) - np.floor(255 * P + 0.5)) <= 1).all()
    assert stats[0].tolist() == box_of(one.plane(flat, 0, "mask")) and one.outside_is_intact(flat)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refused_calls_write_nothing():
    from uia_hip import _lib
    lib = _lib.lib()
    K, B, S = 2, 2, 8
    logits = torch.zeros(K, B, 2, S, S, device=dev())
    src = torch.full((29,), 9, dtype=torch.uint8, device=dev())
    tail = 4096                                                  # (a misplaced logits pointer below spans 2 KiB: it stays inside this tensor)
    out = torch.full((GUARD + 145 + tail,), SENTINEL, dtype=torch.uint8, device=dev())
    stats = torch.full((B, 8), 77, dtype=torch.int32, device=dev())
    sums = torch.full((B, 2), 77, dtype=torch.int64, device=dev())
    ws_bytes = lib.uia_seg_native_ens_workspace_bytes(B)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev())
    # image 0: 4 x 5, mask 0..20, overlay 20..80, probability 80..100, spread 104..124; image 1: 3 x 3, mask 124..133, no overlay, probability 136..145
    desc = np.array([[0, 4, 5, 0, 20, 80, 104, 0], [20, 3, 3, 124, -1, 136, -1, 0]], dtype=np.int32)
    o = out.data_ptr() + GUARD
    assert o % 8 == 0
    ok = dict(K=K, B=B, S=S, log=logits.data_ptr(), flips=0b0100, t=0.5, src=src.data_ptr(), src_bytes=29, d=desc, out=o, out_bytes=145, ws=ws.data_ptr(), wsb=ws_bytes,
              st=stats.data_ptr(), sm=sums.data_ptr())

    def call(**kw):
        v = dict(ok, **kw)
        return raw_call(v["K"], v["B"], v["S"], v["log"], v["flips"], v["t"], v["src"], v["src_bytes"], v["d"], v["out"], v["out_bytes"], v["ws"], v["wsb"], v["st"],
                        v["sm"])

    def edit(b, w, v):
        d = desc.copy()
        d[b, w] = v
        return d
    cases = [  # everything uia_seg_predict_native refuses
             (dict(B=0), "B=0"), (dict(B=65536), "B=65536"), (dict(S=7), "S=7"), (dict(S=1025), "S=1025"),
             (dict(d=edit(1, 1, 0)), "image 1"), (dict(d=edit(0, 2, 0)), "image 0"), (dict(d=edit(1, 1, 16385)), "image 1"), (dict(d=edit(0, 2, 16385)), "image 0"),
             (dict(log=None), "null"), (dict(out=None), "null"), (dict(ws=None), "null"), (dict(st=None), "null"), (dict(src=None), "image 0"),
             (dict(wsb=ws_bytes - 1), "workspace"), (dict(d=edit(1, 0, 21)), "image 1"), (dict(d=edit(0, 0, -2)), "image 0"), (dict(src_bytes=28), "image 1"),
             (dict(d=edit(1, 3, 137)), "the mask of image 1"), (dict(d=edit(0, 4, 100)), "the overlay of image 0"), (dict(d=edit(0, 3, -1)), "the mask of image 0"),
             (dict(d=edit(1, 3, 19)), "the mask of image 0 overlaps the mask of image 1"), (dict(d=edit(1, 3, 79)), "the overlay of image 0 overlaps the mask of image 1"),
             (dict(out=src.data_ptr() + 28), "of image 0 overlaps src"), (dict(out=logits.data_ptr() + 8), "logits"),
             # the members, the flips, the threshold
             (dict(K=0), "K=0"), (dict(K=17), "K=17"), (dict(K=-1), "K=-1"), (dict(flips=0b10000), "flips"), (dict(K=1, flips=0b0100), "flips"),
             (dict(t=0.0), "threshold"), (dict(t=1.0), "threshold"), (dict(t=-0.25), "threshold"), (dict(t=float("nan")), "threshold"), (dict(t=float("inf")), "threshold"),
             # a map that leaves the buffer
             (dict(out_bytes=144), "the probability map of image 1"), (dict(d=edit(1, 5, 137)), "the probability map of image 1"),
             (dict(d=edit(0, 6, 126)), "the spread map of image 0"), (dict(d=edit(0, 5, -2)), "image 0"), (dict(d=edit(1, 6, -3)), "image 1"),
             # a map that overlaps another range ...
             (dict(d=edit(0, 5, 10)), "the mask of image 0 overlaps the probability map of image 0"),
             (dict(d=edit(0, 5, 61)), "the overlay of image 0 overlaps the probability map of image 0"),
             (dict(d=edit(0, 5, 90)), "the probability map of image 0 overlaps the spread map of image 0"),
             (dict(d=edit(1, 6, 128)), "the mask of image 1 overlaps the spread map of image 1"),
             (dict(d=edit(1, 5, 99)), "the probability map of image 0 overlaps the probability map of image 1"),
             # ... src, logits, stats, sums or the workspace (the pointers of a refused call are never followed)
             (dict(src=o + 80), "the probability map of image 0 overlaps src"), (dict(log=o + 136), "the probability map of image 1 overlaps logits"),
             (dict(st=o + 104), "the spread map of image 0 overlaps stats"), (dict(sm=o + 80), "the probability map of image 0 overlaps sums"),
             (dict(ws=o + 136), "the probability map of image 1 overlaps the workspace"), (dict(sm=stats.data_ptr() + 8), "stats overlaps sums"),
             (dict(sm=sums.data_ptr() + 4), "aligned"),
             # the reserved word
             (dict(d=edit(1, 7, 1)), "image 1 has a non-zero reserved"), (dict(d=edit(0, 7, -1)), "image 0 has a non-zero reserved")]
    for kw, word in cases:
        rc, err = call(**kw)
        assert rc != 0 and word in err and "uia_seg_predict_native_ens" in err, (kw, rc, err)
    assert bool((out == SENTINEL).all()) and bool((stats == 77).all()) and bool((sums == 77).all()) and bool((src == 9).all()) and not logits.any()
    rc, err = call()                                             # the same call with nothing wrong runs: z = 0 everywhere, so P = 1/2 exactly
    assert rc == 0, err
    flat = out.cpu().numpy()[GUARD:GUARD + 145]
    assert bool((out[:GUARD] == SENTINEL).all()) and bool((out[GUARD + 145:] == SENTINEL).all())
    assert not flat[0:20].any() and (flat[20:80] == 9).all() and (flat[80:100] == 128).all() and not flat[104:124].any()
    assert not flat[124:133].any() and (flat[136:145] == 128).all() and (flat[100:104] == SENTINEL).all() and (flat[133:136] == SENTINEL).all()
    assert stats.cpu().tolist() == [EMPTY, EMPTY] and sums.cpu().tolist() == [[0, 0], [0, 0]]


def test_python_wrapper_refuses_host_tensors_and_wrong_shapes():
    from uia_hip import ops
    logits = torch.zeros(2, 1, 2, 8, 8, device=dev())
    out = torch.zeros(192, dtype=torch.uint8, device=dev())
    desc = torch.tensor([[-1, 8, 8, 0, -1, 64, 128, 0]], dtype=torch.int32)
    with pytest.raises(ops.UiaError):
        ops.seg_predict_native_ens(logits.cpu(), [0, 0], None, desc, out)
    with pytest.raises(ops.UiaError, match="desc"):
        ops.seg_predict_native_ens(logits, [0, 0], None, desc.to(dev()), out)
    with pytest.raises(ops.UiaError, match="logits"):
        ops.seg_predict_native_ens(logits[0], [0], None, desc, out)
    with pytest.raises(ops.UiaError, match="flips"):
        ops.seg_predict_native_ens(logits, [0, 4], None, desc, out)
    with pytest.raises(ops.UiaError, match="2 members"):
        ops.seg_predict_native_ens(logits, [0], None, desc, out)
    with pytest.raises(ops.UiaError, match="threshold"):
        ops.seg_predict_native_ens(logits, [0, 1], None, desc, out, threshold=1.0)
    with pytest.raises(ops.UiaError, match="sums"):
        ops.seg_predict_native_ens(logits, [0, 1], None, desc, out, sums=torch.zeros(1, 2, dtype=torch.int32, device=dev()))
    with pytest.raises(ops.UiaError, match="leaves the output buffer"):
        ops.seg_predict_native_ens(logits, [0, 1], None, desc, out[:191])
    stats, sums = ops.seg_predict_native_ens(logits, [0, 1], None, desc, out)
    assert stats.cpu().tolist() == [EMPTY] and sums.cpu().tolist() == [[0, 0]] and bool((out[64:128] == 128).all()) and not bool(out[128:].any())
