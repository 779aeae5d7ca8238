"""Float64 restatements of the small kernels around the GEMMs, and the bounds that judge them.

A plain module, no pytest: tests/test_helpers_contract_gpu.py runs the HIP kernels of csrc/decoder.hip, csrc/heads.hip and
csrc/elementwise.hip next to these functions, tests/test_helpers_reference_host.py checks each restatement against a second,
independent form and shows that the bounds catch planted bugs on the CPU.

Every function takes CPU tensors holding exactly the operands the kernel sees (bf16 inputs already rounded, then upcast), and
returns float64 (or, for pure data movement, the exact values in the kernel's storage type).  Layouts follow the kernels:
token-major rows [B·n, ld] for the decoder / head maps, NCHW images, row-major weights.

Bounds.  A reduction is judged element-wise by  |k − ref| ≤ C·u·mag + u_out·|ref|,  with mag the sum of the absolute values of
the terms that make up the element.  Every kernel here does its arithmetic in fp32 on operands that the reference already holds
exactly, so u is fp32's unit roundoff 2^-24 in both dtypes; u_out is the rounding of the stored result (2^-24 fp32, 2^-8 bf16).
"""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
U = 2.0 ** -24
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
TINY = 2.0 ** -120          # absolute floor for results that underflow fp32's normal range (QuickGELU' at x = -100 is ~1e-72)

# ---- calibrated constants.  Each is about twice the worst error-to-bound ratio measured on the MI355X with the constant set to 1,
#      over every comparison of test_helpers_contract_gpu.py that uses it (worst measured in the comment; both dtypes).  The fp32
#      errors of act_bwd are mostly relative to the result (u_out·|ref| carries them), so its constants sit further above.
C_ACT_GELU = 8.0        # act_bwd GELU:       mag = |dy|·(1 + |x|)   measured 3.07 (fp32; bf16 0.995: its own rounding)
C_ACT_QUICK = 4.0       # act_bwd QuickGELU:  mag = |dy|·s·(1 + 1.702|x|)²   measured 1.93 (fp32; bf16 0.996)
C_LN = 3.0              # ln_affine_bwd dx, dγ, dβ: mag per output, see ln_affine_bwd   measured dβ 1.47, dγ 0.78, dx 0.60
C_FILM = 1.2            # film_fwd y, film_bwd dx / dmul / dadd   measured dmul 0.57, fwd / dx 0.50, dadd 0.46
C_COL2IM = 0.75         # col2im3x3: ≤ 9 terms   measured 0.37
C_UPSAMPLE = 1.5        # upsample fwd / bwd: mag·(1 + max(h, w)) (tap weight error grows with the source coordinate)   measured fwd 0.71, bwd 0.40
C_SEGMENT = 0.7         # segment_mean forward (sequential sum of n)   measured 0.33
C_COLSUM = 0.75         # colsum   measured 0.36
C_EMBED_BWD = 0.9       # embed_bwd (atomic adds of the repeated rows)   measured 0.44
C_DICE_GRAD = 3.2       # dicece dlogits: mag = per-pixel gradient magnitude   measured 1.53
C_DICE_LOSS = 0.25      # dicece loss: mag = dice + CE terms summed   measured 0.11


def bound(ref, mag, c, dtype=torch.float32):
    return c * U * mag + U_OUT[dtype] * ref.abs()


class Checker:
    """Collects element-wise comparisons: check(bar, got, ref, bound, ctx) fails an element when |got - ref| > bound or got is not
    finite; exact(bar, got, want, ctx) wants bit-identical values (NaN where want is NaN).  Every failing comparison is kept with its
    case and worst flat index, and the worst error-to-bound ratio of each bar with where it happened."""

    def __init__(self):
        self.failures = []
        self.worst = {}

    def _note(self, bar, worst, where):
        if worst > self.worst.get(bar, (-1.0, ""))[0]:
            self.worst[bar] = (worst, where)
        if not worst <= 1.0:
            self.failures.append(f"{bar}: {where}: error/bound {worst:.3g}")

    def check(self, bar, got, ref, bound_, ctx):
        got = got.detach().cpu().to(F64).reshape(-1)
        ref, bound_ = ref.to(F64).reshape(-1), bound_.to(F64).reshape(-1)
        if got.numel() != ref.numel():
            self.failures.append(f"{bar}: {ctx}: {got.numel()} elements, expected {ref.numel()}")
            return math.inf
        err = (got - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound_.clamp_min(1e-300))
        ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, math.inf))
        if ratio.numel() == 0:
            return 0.0
        i = int(ratio.argmax())
        worst = float(ratio[i])
        self._note(bar, worst, f"{ctx} index={i} got={float(got[i]):.6g} ref={float(ref[i]):.6g}")
        return worst

    def exact(self, bar, got, want, ctx):
        got, want = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
        if got.numel() != want.numel() or got.dtype != want.dtype:
            self.failures.append(f"{bar}: {ctx}: got {got.numel()} x {got.dtype}, expected {want.numel()} x {want.dtype}")
            return
        if got.is_floating_point():
            same = (got == want) | (torch.isnan(got) & torch.isnan(want))
            same &= (torch.signbit(got) == torch.signbit(want)) | torch.isnan(want)
        else:
            same = got == want
        if not bool(same.all()):
            i = int((~same).nonzero()[0])
            self.failures.append(f"{bar}: {ctx}: {int((~same).sum())} elements differ, first index={i} got={got[i].item()} want={want[i].item()}")

    def fail(self, bar, ctx, what):
        self.failures.append(f"{bar}: {ctx}: {what}")

    def ok(self):
        return not self.failures

    def report(self, limit=40):
        lines = [f"{len(self.failures)} failing comparisons"] + self.failures[:limit]
        lines += ["worst error/bound per bar:"] + [f"  {k}: {v[0]:.3g} at {v[1]}" for k, v in sorted(self.worst.items())]
        return "\n".join(lines)


# ------------------------------------------------------------------------------------------ data movement (exact)
def im2col3x3(x, h, w, tok_off):
    """x [B, ntok, C] → [B·h·w, 9C]: row (b, y, x), column (ky·3 + kx)·C + c = x[b, tok_off + (y+ky-1)·w + (x+kx-1), c], zero
    outside the grid.  Built from F.unfold (its columns run (c, ky, kx))."""
    B, _, C = x.shape
    img = x[:, tok_off:tok_off + h * w].reshape(B, h, w, C).permute(0, 3, 1, 2)
    u = F.unfold(img, 3, padding=1)                                    # [B, C·9, h·w]
    return u.reshape(B, C, 9, h * w).permute(0, 3, 2, 1).reshape(B * h * w, 9 * C)


def col2im3x3(dcols, B, h, w, C, ntok, tok_off):
    """The adjoint of im2col3x3: [B·h·w, 9C] → [B, ntok, C], rows outside tok_off .. tok_off + h·w zero.  Built from F.fold."""
    u = dcols.reshape(B, h * w, 9, C).permute(0, 3, 2, 1).reshape(B, C * 9, h * w)
    img = F.fold(u, (h, w), 3, padding=1)                              # [B, C, h, w]
    out = torch.zeros(B, ntok, C, dtype=dcols.dtype)
    out[:, tok_off:tok_off + h * w] = img.permute(0, 2, 3, 1).reshape(B, h * w, C)
    return out


def unshuffle(tmp, B, h, w, k1, k2):
    """tmp [B·h·w·k1², ≥k2²] → [B, h·k1·k2, w·k1·k2]: tmp row ((b·h + y)·w + x)·k1² + i·k1 + j, column i2·k2 + j2 is pixel
    (y·k1 + i)·k2 + i2, (x·k1 + j)·k2 + j2 of image b."""
    t = tmp[:, :k2 * k2].reshape(B, h, w, k1, k1, k2, k2)              # b y x i j i2 j2
    return t.permute(0, 1, 3, 5, 2, 4, 6).reshape(B, h * k1 * k2, w * k1 * k2)


def shuffle(dout, B, h, w, k1, k2, ld):
    """The inverse permutation of unshuffle: [B, H, W] → [B·h·w·k1², ld], columns k2² .. ld zero."""
    t = dout.reshape(B, h, k1, k2, w, k1, k2).permute(0, 1, 4, 2, 5, 3, 6).reshape(B * h * w * k1 * k1, k2 * k2)
    out = torch.zeros(t.shape[0], ld, dtype=dout.dtype)
    out[:, :k2 * k2] = t
    return out


def im2col(img, P, ldo=None):
    """Conv2d(k = P, s = P) patches: img [B, C, H, W] → [B·gh·gw, ldo], column (c·P + ky)·P + kx, zero beyond C·P²."""
    B, C, H, W = img.shape
    u = F.unfold(img, P, stride=P).transpose(1, 2).reshape(B * (H // P) * (W // P), C * P * P)
    if ldo is None or ldo == C * P * P:
        return u
    out = torch.zeros(u.shape[0], ldo, dtype=img.dtype)
    out[:, :u.shape[1]] = u
    return out


def embed(ids, pos_idx, table, pos, type0):
    """out[r] = table[ids[r]] + pos[pos_idx[r]] (+ type0), each sum in fp32 as the kernel adds (table + pos, then + type0); a row whose
    id or position lies outside its table is NaN."""
    V, P = table.shape[0], pos.shape[0]
    ok = (ids >= 0) & (ids < V) & (pos_idx >= 0) & (pos_idx < P)
    out = table[ids.clamp(0, V - 1)] + pos[pos_idx.clamp(0, P - 1)]
    if type0 is not None:
        out = out + type0
    out[~ok] = float("nan")
    return out


def pack_weights(src, scale, RP, CP, g, dtype):
    """The four operand forms of pack_weights, written out with plain indexing: dict of flat tensors of RP·CP elements (only the
    source's R×C elements set; the rest stays NaN, for the caller's own padding).  g = 64 bytes / element size."""
    R, C = src.shape
    v = (src * (scale if scale != 0 else 1.0)).to(dtype).reshape(-1)
    r = torch.arange(R).repeat_interleave(C)                # element (r, c) of the source, row-major
    c = torch.arange(C).repeat(R)
    out = {k: torch.full((RP * CP,), float("nan"), dtype=dtype) for k in ("row", "row_kb", "tr", "tr_kb")}
    out["row"][r * CP + c] = v
    out["row_kb"][((c // g) * RP + r) * g + c % g] = v
    out["tr"][c * RP + r] = v
    out["tr_kb"][((r // g) * CP + c) * g + r % g] = v
    return out


# ------------------------------------------------------------------------------------------ elementwise
def act_bwd(dy, x, act):
    """dy · act'(x) in float64 through autograd: x is the pre-activation for "gelu" (F.gelu, exact erf) and "quick_gelu"
    (x·σ(1.702x)), the post-activation for "relu" (d = dy where y > 0)."""
    dy, x = dy.to(F64), x.to(F64)
    if act in (None, "none"):
        return dy.clone()
    if act == "relu":
        return torch.where(x > 0, dy, torch.zeros_like(dy))
    xx = x.clone().requires_grad_(True)
    y = F.gelu(xx) if act == "gelu" else xx * torch.sigmoid(1.702 * xx)
    y.backward(dy)
    return xx.grad


def act_bwd_mag(dy, x, act):
    dy, x = dy.to(F64).abs(), x.to(F64)
    if act == "gelu":
        return dy * (1 + x.abs()) + TINY / U
    a = 1.702 * x
    return dy * torch.sigmoid(a) * (1 + a.abs()) ** 2 + TINY / U


# ------------------------------------------------------------------------------------------ reductions
def ln_affine_bwd(dy, x, gamma, eps, dres=None):
    """LayerNorm backward with dγ, dβ via autograd of F.layer_norm: (dx [+ dres], dγ, dβ) and the magnitudes of their terms
    (dx: rstd·(|g| + mean|g| + |xhat|·mean|g·xhat|)·√D, with g = dy·γ; dγ: Σ|dy·xhat|·(1 + √D); both times the row's centring
    condition 1 + max|x|·rstd; dβ: Σ|dy|)."""
    M, D = x.shape
    dy, x, gamma = dy.to(F64), x.to(F64), gamma.to(F64)
    xx, gg, bb = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), torch.zeros(D, dtype=F64, requires_grad=True)
    F.layer_norm(xx, (D,), gg, bb, eps).backward(dy)
    dx = xx.grad + (dres.to(F64) if dres is not None else 0)
    mu = x.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    xhat = (x - mu) * rstd
    g = (dy * gamma).abs()
    cond = 1 + x.abs().amax(1, keepdim=True) * rstd        # x − mean cancels: its error is u·|x|, i.e. u·|x|·rstd relative to xhat
    mag_dx = rstd * (g + g.mean(1, keepdim=True) + xhat.abs() * (g * xhat.abs()).mean(1, keepdim=True)) * D ** 0.5 * cond
    mag_dx = mag_dx + (dres.to(F64).abs() if dres is not None else 0)
    mag_dg = ((dy * xhat).abs() * (1 + D ** 0.5) * cond).sum(0)
    mag_db = dy.abs().sum(0)
    return dict(dx=dx, dg=gg.grad, db=bb.grad, mag_dx=mag_dx, mag_dg=mag_dg, mag_db=mag_db)


def film_fwd(x, mul, add):
    """y[b, n, c] = mul[b, c]·x[b, n, c] + add[b, c]; magnitude |mul·x| + |add|."""
    x, mul, add = x.to(F64), mul.to(F64)[:, None], add.to(F64)[:, None]
    return mul * x + add, (mul * x).abs() + add.abs()


def film_bwd(dy, x, mul):
    """(dx, dmul, dadd) of film_fwd and the magnitudes of dmul / dadd."""
    dy, x, mul = dy.to(F64), x.to(F64), mul.to(F64)
    return dict(dx=dy * mul[:, None], dmul=(dy * x).sum(1), dadd=dy.sum(1), mag_dx=(dy * mul[:, None]).abs(),
                mag_dmul=(dy * x).abs().sum(1) * (1 + dy.shape[1] ** 0.5), mag_dadd=dy.abs().sum(1) * (1 + dy.shape[1] ** 0.5))


def col2im3x3_mag(dcols, B, h, w, C, ntok, tok_off):
    return col2im3x3(dcols.abs(), B, h, w, C, ntok, tok_off) * 9


def tokens_to_image(tok, B, C, h, w):
    """token-major [B·h·w, ld ≥ C] → [B, C, h, w] (float64)."""
    return tok[:, :C].to(F64).reshape(B, h, w, C).permute(0, 3, 1, 2)


def image_to_tokens(img):
    B, C, h, w = img.shape
    return img.permute(0, 2, 3, 1).reshape(B * h * w, C)


def upsample(img, H, W):
    """nn.Upsample((H, W), mode="bilinear", align_corners=False) in float64."""
    return F.interpolate(img.to(F64), size=(H, W), mode="bilinear", align_corners=False)


def upsample_bwd(dout, h, w):
    """The gradient of upsample with respect to its [B, C, h, w] input, by autograd."""
    B, C = dout.shape[:2]
    x = torch.zeros(B, C, h, w, dtype=F64, requires_grad=True)
    upsample(x, dout.shape[2], dout.shape[3]).backward(dout.to(F64))
    return x.grad


def taps_1d(n_out, n_in):
    """PyTorch's align_corners=False source index, written out: [n_out, n_in] interpolation matrix and the 'may tap' indicator
    (every input within 1.5 of the source coordinate: it also holds the neighbours an fp32 floor can pick instead)."""
    Wm = torch.zeros(n_out, n_in, dtype=F64)
    Im = torch.zeros(n_out, n_in, dtype=F64)
    scale = n_in / n_out
    for o in range(n_out):
        s = max(scale * (o + 0.5) - 0.5, 0.0)
        i0 = min(int(math.floor(s)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l1 = s - i0
        Wm[o, i0] += 1 - l1
        Wm[o, i1] += l1
        for i in range(n_in):
            if abs(i - s) < 1.5 or i == i0:
                Im[o, i] = 1
    return Wm, Im


def upsample_taps(img, H, W):
    """upsample from the hand-written separable taps: Ry · img · Rxᵀ."""
    Ry, _ = taps_1d(H, img.shape[2])
    Rx, _ = taps_1d(W, img.shape[3])
    return Ry @ img.to(F64) @ Rx.T


def upsample_mag(img, H, W, backward=False):
    """Σ |terms| bounding each output (forward: the taps of an output; backward: the outputs that may tap an input),
    times (1 + max source coordinate): the tap weights carry an absolute error of a few u·s."""
    if backward:
        h, w = H, W
        _, Iy = taps_1d(img.shape[2], h)
        _, Ix = taps_1d(img.shape[3], w)
        m = Iy.T @ img.to(F64).abs() @ Ix
    else:
        h, w = img.shape[2], img.shape[3]
        _, Iy = taps_1d(H, h)
        _, Ix = taps_1d(W, w)
        m = Iy @ img.to(F64).abs() @ Ix.T
    return m * (1 + max(h, w))


def segment_mean(x, B, n, C):
    """mean over each image's n token rows: x [B·n, ld ≥ C] → ([B, C], magnitude Σ|x|/n)."""
    t = x[:, :C].to(F64).reshape(B, n, C)
    return t.mean(1), t.abs().sum(1) / n * (1 + n)


def colsum(a):
    """Column sums in float64 and their magnitude Σ_m |a[m, :]|·(4 + √M) (a thread's sequential run, a 4-way tree, one atomic
    add per 1024-row chunk: the √M growth of a random-walk rounding error)."""
    a = a.to(F64)
    M = a.shape[0]
    return a.sum(0), a.abs().sum(0) * (4 + math.sqrt(M))


def embed_bwd(ids, dx, vocab, pad_id):
    """dtable[ids[r]] += dx[r] for ids in [0, vocab) other than pad_id (index_add_), and the magnitude Σ|dx| of each row."""
    dx = dx.to(F64)
    keep = (ids != pad_id) & (ids >= 0) & (ids < vocab)
    out = torch.zeros(vocab, dx.shape[1], dtype=F64)
    mag = torch.zeros(vocab, dx.shape[1], dtype=F64)
    out.index_add_(0, ids[keep], dx[keep])
    mag.index_add_(0, ids[keep], dx[keep].abs())
    return out, mag * (1 + math.sqrt(max(1, int(keep.sum()))))


def dicece(logits, label, nr=1e-8, dr=1e-8):
    """oracle.losses_ref.dice_ce (MONAI DiceCELoss, softmax, squared_pred, one-hot labels) in float64, its gradient by autograd,
    and magnitudes: per element |p·(g − Σ g p)| terms and the CE term; for the loss, its dice and CE parts' absolute sums."""
    from oracle import losses_ref
    z = logits.to(F64).clone().requires_grad_(True)
    loss = losses_ref.dice_ce(z, label.to(F64), nr, dr)
    loss.backward()
    B, C = logits.shape[:2]
    HW = logits.shape[2] * logits.shape[3]
    p = torch.softmax(logits.to(F64), 1)
    t = F.one_hot(label[:, 0].long(), C).permute(0, 3, 1, 2).to(F64)
    den = (p * p).sum((2, 3)) + t.sum((2, 3)) + dr
    inter = (p * t).sum((2, 3))
    a1 = (2 / (B * C)) * (2 * inter + nr) / den ** 2
    a2 = (2 / (B * C)) / den
    g = (a1[:, :, None, None] * p).abs() + a2[:, :, None, None] * t
    gp = (g * p).sum(1, keepdim=True)
    # the per-image sums I, P², T come from HW terms: their relative error (≲ √HW·u) reaches every pixel's g
    # __expf / __logf carry a relative error that grows with their argument: the spread of the pixel's logits
    spread = 2 + (logits.amax(1, keepdim=True) - logits.amin(1, keepdim=True)).to(F64)
    mag = ((p * (g + gp)) * (1 + math.sqrt(HW)) + (p + t) / (B * HW)) * spread
    ce = -torch.log_softmax(logits.to(F64), 1).gather(1, label.long())
    mag_loss = float(1 + math.sqrt(B * C + HW)) * (1.0 + float(ce.abs().sum()) / (B * HW) + float(((2 * inter + nr) / den).abs().sum()) / (B * C))
    return float(loss.detach()), z.grad, mag, mag_loss
