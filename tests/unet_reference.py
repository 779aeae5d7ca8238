"""Float64 restatement of the reference's DINOv2 UNet segmentation decoder (src/third_party/dino/dinov2.py:130-260, UNetDecoder with
resize_image=True), on a state dict with the reference's key names (`up{1..4}.{upconv,conv.0,conv.1,skip_conv.0,skip_conv.1}.*`).

    block(x, skip) = CBR_conv(cat[ConvT2x2(x), Upsample_ac(CBR_skip(skip), a.H / 37)])     CBR = ReLU(BatchNorm2d(Conv2d 3x3 pad 1 + bias))
    decoder        = resize(up4(up3(up2(up1(blk11, blk10), blk9), blk8), blk7))              resize = bicubic, antialias, align_corners=False

BatchNorm: batch mean / biased variance in training (running buffers updated with the unbiased variance, momentum 0.1), running statistics in eval.
The logits have passed through the last block's BatchNorm + ReLU before the resize, as in the reference.

Also the seeded weights and inputs of the small golden geometry (tools/gen_dino_seg_golden.py records the reference's outputs on them).
A plain module, no pytest: tests/test_dino_seg_host.py checks it against tests/golden/dino_seg_small.npz, tests/test_dino_seg_gpu.py runs the kernels
against it.

The second half restates each kernel of csrc/unet_conv.hip, csrc/unet_bn.hip and csrc/unet_resample.hip on its own, element by element, with the
magnitudes and constants that bound it: tests/test_unet_reference_host.py checks these against PyTorch's own float64 ops,
tests/test_unet_contract_gpu.py runs the kernels against them."""
import torch
import torch.nn.functional as F

F64 = torch.float64

# the small golden geometry: embed 64, 84 px at patch 14 -> 6 x 6 maps, grids 12 / 24 / 48 / 96, resize 96 -> 84
SMALL = dict(embed_dim=64, image_size=84, patch_size=14, num_classes=3, batch=2, seed=4321)


def state_shapes(embed_dim, num_classes):
    """(name, shape) of UNetDecoder(embed_dim, num_classes) in the reference's state-dict order (BatchNorm buffers included)."""
    out = []
    chans = [embed_dim, embed_dim // 2, embed_dim // 4, embed_dim // 8, num_classes]
    for i in range(4):
        cin, cout = chans[i], chans[i + 1]
        p = f"up{i + 1}."
        out += [(p + "upconv.weight", (cin, cout, 2, 2)), (p + "upconv.bias", (cout,))]
        for name, c_in in (("conv", 2 * cout), ("skip_conv", embed_dim)):
            out += [(p + name + ".0.weight", (cout, c_in, 3, 3)), (p + name + ".0.bias", (cout,)), (p + name + ".1.weight", (cout,)),
                    (p + name + ".1.bias", (cout,)), (p + name + ".1.running_mean", (cout,)), (p + name + ".1.running_var", (cout,)),
                    (p + name + ".1.num_batches_tracked", ())]
    return out


def seeded_state(embed_dim, num_classes, seed):
    """Weights drawn from one CPU generator in key order: convs N(0, 1/fan_in), biases N(0, 0.1²), BN γ = 1 + N(0, 0.1²), β N(0, 0.1²);
    running_mean 0, running_var 1, num_batches_tracked 0 (a fresh module's buffers)."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for k, shp in state_shapes(embed_dim, num_classes):
        if k.endswith("num_batches_tracked"):
            P[k] = torch.zeros((), dtype=torch.int64)
        elif k.endswith("running_mean"):
            P[k] = torch.zeros(shp, dtype=F64)
        elif k.endswith("running_var"):
            P[k] = torch.ones(shp, dtype=F64)
        elif k.endswith(".1.weight"):
            P[k] = 1.0 + 0.1 * torch.randn(shp, generator=g, dtype=F64)
        elif k.endswith("bias"):
            P[k] = 0.1 * torch.randn(shp, generator=g, dtype=F64)
        else:
            fan_in = shp[0] * 4 if "upconv" in k else shp[1] * 9
            P[k] = torch.randn(shp, generator=g, dtype=F64) / fan_in ** 0.5
    return P


def seeded_inputs(embed_dim, image_size, patch_size, num_classes, batch, seed):
    """The five patch-token maps [B, h·w, D] (blocks 7..11 in order) and the upstream gradient of the logits [B, C, S, S]."""
    g = torch.Generator().manual_seed(seed + 1)
    h = image_size // patch_size
    maps = [torch.randn(batch, h * h, embed_dim, generator=g, dtype=F64) for _ in range(5)]
    dlogits = torch.randn(batch, num_classes, image_size, image_size, generator=g, dtype=F64)
    return maps, dlogits


def resize(x, size):
    """What torchvision 0.24's transforms.Resize(size, BICUBIC) runs on a float tensor."""
    return F.interpolate(x, size=size, mode="bicubic", align_corners=False, antialias=True)


def _cbr(P, p, x, training, bufs):
    y = F.conv2d(x, P[p + ".0.weight"], P[p + ".0.bias"], padding=1)
    rm, rv = bufs[p + ".1.running_mean"], bufs[p + ".1.running_var"]
    if training:
        n = y.shape[0] * y.shape[2] * y.shape[3]
        mean = y.mean(dim=(0, 2, 3))
        var = y.var(dim=(0, 2, 3), unbiased=False)
        bufs[p + ".1.running_mean"] = 0.9 * rm + 0.1 * mean
        bufs[p + ".1.running_var"] = 0.9 * rv + 0.1 * var * n / (n - 1)
        bufs[p + ".1.num_batches_tracked"] = bufs[p + ".1.num_batches_tracked"] + 1
    else:
        mean, var = rm, rv
    z = (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + 1e-5) * P[p + ".1.weight"][None, :, None, None] + P[p + ".1.bias"][None, :, None, None]
    return torch.relu(z)


def decoder_forward(P, maps, image_size, patch_size, training=True, bufs=None):
    """UNetDecoder(resize_image=True) on the five patch maps (blocks 7..11, [B, h·w, D] each).  bufs: the BatchNorm buffers (a dict, updated in
    place in training; default: those of P).  Returns (logits [B, C, S, S], bufs)."""
    bufs = {k: v.clone() for k, v in P.items() if "running" in k or "num_batches" in k} if bufs is None else bufs
    h = image_size // patch_size
    D = maps[0].shape[2]
    nchw = [m.reshape(-1, h, h, D).permute(0, 3, 1, 2) for m in maps]
    skip4, skip3, skip2, skip1, x = nchw
    for i, skip in enumerate((skip1, skip2, skip3, skip4)):
        p = f"up{i + 1}."
        a = F.conv_transpose2d(x, P[p + "upconv.weight"], P[p + "upconv.bias"], stride=2)
        s = _cbr(P, p + "skip_conv", skip, training, bufs)
        s = F.interpolate(s, scale_factor=a.shape[2] / skip.shape[2], mode="bilinear", align_corners=True)
        x = _cbr(P, p + "conv", torch.cat([a, s], dim=1), training, bufs)
    return resize(x, (image_size, image_size)), bufs


# ====================================================================================================================================
# Per-kernel restatements.  Every function takes CPU tensors holding exactly the operands the kernel sees (already rounded to the compute
# dtype, NHWC, weights in the kernel's row layout) and returns (ref, mag): ref in float64, mag the same expression with every operand and
# every tap weight replaced by its absolute value.  The judge is helpers_reference.bound(ref, mag, c, dtype) = c·2⁻²⁴·mag + u_out·|ref|.
#
# Constants.  None is tuned on a kernel: each c is the derivable worst case, the number of fp32 roundings on the longest accumulation chain
# of that kernel at that shape (a function of the shape where the chain is).  Beside each stands the kernels' measured worst error/bound on
# the MI355X over tests/test_unet_contract_gpu.py (which prints them per bar when run with -s): records, not inputs.  In bf16 the worst
# element of every stored tensor sits at 0.94 .. 0.996: that is the rounding of the result itself (u_out·|ref|), so the fp32 figure is given.
# ====================================================================================================================================
def c_conv(taps, cin):
    """uia_conv_igemm: taps·Cin products added one after another (the direct kernel's fmaf chain; the MFMA forms add in blocks, fewer
    roundings), the bias and one spare.   measured: fp32 forward 0.016, dgrad 0.11, transposed forward 0.20, backward 0.16 (direct kernel, few channels)"""
    return taps * cin + 2


def c_wgrad(M, splits):
    """uia_conv_wgrad: the M pixels of a split added in order, then the splits.   measured conv3x3 0.194 (M = 1), convt 0.254"""
    return M + splits + 2


def bn_slices(M):
    return min((M + 255) // 256, 256)                   # slices_for(M) with UIA_BN_SLICES = 256


def c_reduce(M, C):
    """reduce_kernel + finalize: the rows one thread adds, the row lanes added after them, the slices, and 8 for the handful of roundings
    around the sums.  reduce_kernel adds the RP row lanes one after another in lane order (`for k = 1 .. RP − 1: a += red[tid + k·Cb]`, no
    tree: 255 additions in a row at C = 1), and col_finalize_kernel the slices one after another, so these are the kernel's own chains
    (bn_finalize_kernel combines the slices in double: no fp32 rounding there, the term is kept for the two fp32 sums).  The 8: (the shift by K, x̂, the affine and the running-buffer blend).
    measured: mean 0.092, invstd 0.064, scale 0.055, shift 0.069, running mean 0.179, running var 0.11, out fp32 0.052; under a mean of ±1000
    invstd 0.007, mean 0.004; backward dβ 0.011, dγ 0.189, dy fp32 0.10; colsum 0.091"""
    S = bn_slices(M)
    per = (M + S - 1) // S
    RP = 256 // min(C, 256)
    return (per + RP - 1) // RP + (RP - 1) + (S - 1) + 8


C_BN_EVAL = 12.0            # measured fp32 0.23.   g = γ / sqrtf(var + eps) (add, sqrt ≤ 1 ulp, divide ≤ 2.5 ulp), shift = β − mean·g (2), the fma (1): mag = |y·g| + |β| + |mean·g|
C_UPSAMPLE_AC = 8.0         # measured fp32 0.048.   forward: 7 roundings of the 4-tap blend; each tap weight is off by ≤ 2u·src ≤ 2u·extent per axis -> mag·(1 + extent)
# uia_resize_aa, on mag = |Wy|·|x|·|Wx|ᵀ·(1 + the largest of the four extents).  The tap count of the two passes (7 .. 16 forward, 5 .. 15
# backward at the test's shapes) is no ceiling here: a tap's fp32 weight is off by an absolute amount of a few u however small the weight is
# (the cubic's Horner form has terms up to 4 next to its zeros at |x| = 1 and 2), so an element whose large operand meets a near-zero weight
# errs by more than taps·u·Σ|w·x|.  PyTorch's own fp32 CPU resize, which forms its weights the same way, shows it: against the float64
# restatement on the test's inputs its worst error is 5.2·u·mag forward and 13.1·u·mag backward (1x11 -> 1x7: a weight of −0.0024, off by
# 4.5u, meets a gradient of −2.2).  So the constants are four times those figures, as the sums of the kernel run in another order.
C_RESIZE_AA = 21.0          # forward    measured 0.25
C_RESIZE_AA_BWD = 53.0      # backward   measured fp32 0.25


def c_upsample_ac_bwd(f):
    """the gather adds at most 2f + 3 outputs per axis in a row, on top of the forward's terms.   measured fp32 0.024"""
    return 4.0 * f + 12.0


def _shift(x, dy, dx):
    """s[b, y, x] = x[b, y + dy, x + dx], zero outside the grid."""
    H, W = x.shape[1], x.shape[2]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return xp[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def _split(t, n1):
    return t if n1 is None or n1 == t.shape[-1] else (t[..., :n1], t[..., n1:])


def _cat(x1, x2, dt):
    return x1.to(dt) if x2 is None else torch.cat([x1.to(dt), x2.to(dt)], dim=3)


def _conv3(x, w, bias):
    N, Cin = w.shape[0], x.shape[3]
    w = w.reshape(N, 9, Cin)
    out = torch.zeros(*x.shape[:3], N, dtype=x.dtype)
    for t in range(9):
        out = out + _shift(x, t // 3 - 1, t % 3 - 1) @ w[:, t].T
    return out if bias is None else out + bias


def conv3x3(x1, x2, w, bias=None, n1=None, dt=F64):
    """UIA_CONV3: x1 [B,H,W,C1] (+ x2 [B,H,W,C2]), w [N, 9·(C1+C2)] (k = tap·Cin + c), bias [N] -> [B,H,W,N], split at channel n1."""
    x, w = _cat(x1, x2, dt), w.to(dt)
    b = None if bias is None else bias.to(dt)
    ref = _conv3(x, w, b)
    mag = _conv3(x.abs(), w.abs(), None if b is None else b.abs())
    return _split(ref, n1), _split(mag, n1)


def conv3_dgrad_rows(w, cin):
    """The rows the data gradient feeds to UIA_CONV3: w [N, 9·Cin] -> [Cin, 9·N], taps flipped."""
    N = w.shape[0]
    return w.reshape(N, 9, cin).flip(1).permute(2, 1, 0).reshape(cin, 9 * N).contiguous()


def conv3x3_dgrad(dy, w, n1=None, dt=F64):
    """The gradient of conv3x3 with respect to cat(x1, x2): dx[b, y, x, c] = Σ_t Σ_n dy[b, y − dy_t, x − dx_t, n]·w[n, t, c], split at n1 = C1."""
    N = dy.shape[3]
    Cin = w.shape[1] // 9
    wt = w.to(dt).reshape(N, 9, Cin)

    def run(g, ww):
        out = torch.zeros(*g.shape[:3], Cin, dtype=dt)
        for t in range(9):
            out = out + _shift(g, 1 - t // 3, 1 - t % 3) @ ww[:, t]
        return out
    return _split(run(dy.to(dt), wt), n1), _split(run(dy.to(dt).abs(), wt.abs()), n1)


def conv3x3_wgrad(x1, x2, dy, dt=F64):
    """dW[n, t·Cin + c] = Σ_{b,y,x} dy[b, y, x, n]·cat(x1, x2)[b, y + dy_t, x + dx_t, c]."""
    x, g = _cat(x1, x2, dt), dy.to(dt)
    N, Cin = g.shape[3], x.shape[3]

    def run(xx, gg):
        return torch.stack([torch.einsum("bhwn,bhwc->nc", gg, _shift(xx, t // 3 - 1, t % 3 - 1)) for t in range(9)], dim=1).reshape(N, 9 * Cin)
    return run(x, g), run(x.abs(), g.abs())


def _quad(t, di, dj):
    return t[:, di::2, dj::2]


def convt_fwd(x, w, bias=None, dt=F64):
    """UIA_CONVT_FWD: x [B,h,w,Cin], w [4·Cout, Cin] (row (2·di + dj)·Cout + o), bias [Cout] -> [B,2h,2w,Cout]."""
    B, h, ww, _ = x.shape
    Cout = w.shape[0] // 4

    def run(xx, wt, b):
        out = torch.zeros(B, 2 * h, 2 * ww, Cout, dtype=dt)
        for t in range(4):
            _quad(out, t >> 1, t & 1).copy_(xx @ wt[t * Cout:(t + 1) * Cout].T)
        return out if b is None else out + b
    b = None if bias is None else bias.to(dt)
    return run(x.to(dt), w.to(dt), b), run(x.to(dt).abs(), w.to(dt).abs(), None if b is None else b.abs())


def convt_bwd(dy, w, dt=F64):
    """UIA_CONVT_BWD: dy [B,2h,2w,Cout], w [Cin, 4·Cout] (column (2·di + dj)·Cout + o) -> dx [B,h,w,Cin]."""
    Cout = dy.shape[3]

    def run(g, wt):
        return sum(_quad(g, t >> 1, t & 1) @ wt[:, t * Cout:(t + 1) * Cout].T for t in range(4))
    return run(dy.to(dt), w.to(dt)), run(dy.to(dt).abs(), w.to(dt).abs())


def convt_wgrad(x, dy, dt=F64):
    """G[(2·di + dj)·Cout + o, c] = Σ_{b,y,x} dy[b, 2y + di, 2x + dj, o]·x[b, y, x, c]."""
    def run(xx, g):
        return torch.cat([torch.einsum("bhwo,bhwc->oc", _quad(g, t >> 1, t & 1), xx) for t in range(4)], dim=0)
    return run(x.to(dt), dy.to(dt)), run(x.to(dt).abs(), dy.to(dt).abs())


# ---------------------------------------------------------------------------------------------------------------- BatchNorm, column sums
def f32(v):
    """A Python float as the kernel receives it through a float argument."""
    return float(torch.tensor(v, dtype=torch.float32))


def bn_train(y, gamma, beta, run_mean, run_var, nbt, momentum, eps, relu=True):
    """Train-mode BatchNorm (+ ReLU) on rows y [M, C].  Returns a dict of (ref, mag) pairs: mean, invstd, scale, shift, out, and run_mean,
    run_var (unbiased variance, blended with momentum; None without buffers), and nbt = num_batches_tracked + 1 (None without it).
    The magnitudes follow the kernel's shifted sums: slice s of the rows (bn_slices(M) contiguous runs) is summed as Σ(y − K), Σ(y − K)² with K
    the slice's first row, so the mean's terms are |y − K|/M and the variance's (y − K)²/M: 3 of them (q, and a²/n ≤ Σ|d|·Σ|d|/n twice over) plus
    the between-slice terms 2·|mean_s − mean|·Σ|y − K|/M of Chan's combination.  A kernel that summed y² unshifted has terms y²/M instead,
    and fails this bound once the mean is large.  momentum and eps are the float arguments (f32(·))."""
    y, gamma, beta = y.to(F64), gamma.to(F64), beta.to(F64)
    M, C = y.shape
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    S = bn_slices(M)
    per = (M + S - 1) // S
    mag_mean, mag_var = torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64)
    for s in range(S):
        ys = y[s * per:min((s + 1) * per, M)]
        if ys.shape[0] == 0:
            continue
        d = (ys - ys[0]).abs()
        mag_mean += d.sum(0) / M
        mag_var += (3 * (d * d).sum(0) + 2 * (ys.mean(0) - mean).abs() * d.sum(0)) / M
    invstd = 1 / torch.sqrt(var + eps)
    mag_invstd = 0.5 * invstd ** 3 * mag_var + invstd
    scale = gamma * invstd
    mag_scale = gamma.abs() * mag_invstd + scale.abs()
    shift = beta - mean * scale
    mag_shift = mean.abs() * mag_scale + scale.abs() * (mag_mean + mean.abs()) + beta.abs()
    z = y * scale + shift
    out = torch.relu(z) if relu else z
    mag_out = y.abs() * mag_scale + mag_shift
    r = dict(mean=(mean, mag_mean + mean.abs()), invstd=(invstd, mag_invstd), scale=(scale, mag_scale), shift=(shift, mag_shift), out=(out, mag_out),
             run_mean=None, run_var=None, nbt=None if nbt is None else int(nbt) + 1)
    if run_mean is not None:
        unb = var * M / (M - 1) if M > 1 else var
        rm, rv = run_mean.to(F64), run_var.to(F64)
        r["run_mean"] = ((1 - momentum) * rm + momentum * mean, ((1 - momentum) * rm).abs() + momentum * (mag_mean + mean.abs()))
        r["run_var"] = ((1 - momentum) * rv + momentum * unb, ((1 - momentum) * rv).abs() + momentum * (mag_var * M / max(M - 1, 1) + unb))
    return r


def bn_eval(y, gamma, beta, run_mean, run_var, eps, relu=True):
    """Eval-mode BatchNorm (+ ReLU) on rows y [M, C] with the running statistics: (out, mag) with mag = |y·g| + |β| + |mean·g|."""
    y, gamma, beta, rm, rv = (t.to(F64) for t in (y, gamma, beta, run_mean, run_var))
    g = gamma / torch.sqrt(rv + eps)
    z = y * g + (beta - rm * g)
    return (torch.relu(z) if relu else z), (y * g).abs() + beta.abs() + (rm * g).abs()


def bn_relu_bwd(y, dout, scale, shift, mean, invstd, gamma):
    """Backward of train-mode BatchNorm + ReLU on rows [M, C], from the saved fp32 scale / shift / mean / invstd as the kernel takes them:
    dz = dout·[y·scale + shift > 0], dβ = Σ dz, dγ = Σ dz·x̂ (x̂ = (y − mean)·invstd), dy = γ·invstd·(dz − dβ/M − x̂·dγ/M).
    Returns dict(dy, dgamma, dbeta: (ref, mag) pairs; z: |y·scale + shift| per element; band: the width below which the kernel's fp32 z may
    take the other sign, 2u·(|y·scale| + |shift|): one fma rounding, doubled)."""
    y, dout, scale, shift, mean, invstd, gamma = (t.to(F64) for t in (y, dout, scale, shift, mean, invstd, gamma))
    M = y.shape[0]
    z = y * scale + shift
    dz = torch.where(z > 0, dout, torch.zeros_like(dout))
    xh = (y - mean) * invstd
    dbeta, dgamma = dz.sum(0), (dz * xh).sum(0)
    mag_db, mag_dg = dz.abs().sum(0), (dz * xh).abs().sum(0)
    k = (gamma * invstd).abs()
    dy = gamma * invstd * (dz - dbeta / M - xh * dgamma / M)
    mag_dy = k * (dz.abs() + (mag_db + dbeta.abs()) / M + xh.abs() * (mag_dg + dgamma.abs()) / M)
    return dict(dy=(dy, mag_dy), dgamma=(dgamma, mag_dg), dbeta=(dbeta, mag_db), z=z.abs(), band=2 * 2.0 ** -24 * ((y * scale).abs() + shift.abs()))


def clear_relu_band(y, scale, shift, dtype):
    """y (values of `dtype`) with every element whose |y·scale + shift| lies in bn_relu_bwd's band moved out of it, still values of `dtype`."""
    y = y.clone()
    for _ in range(8):
        yd = y.to(F64)
        z = yd * scale.to(F64) + shift.to(F64)
        bad = z.abs() <= 4 * 2.0 ** -24 * ((yd * scale.to(F64)).abs() + shift.to(F64).abs())
        if not bool(bad.any()):
            return y
        y = torch.where(bad, (yd * 1.0625 + 0.0625).to(dtype).to(y.dtype), y)
    raise AssertionError("clear_relu_band: elements left in the band")


def colsum(y):
    """Column sums of rows [M, C] and Σ|y|."""
    y = y.to(F64)
    return y.sum(0), y.abs().sum(0)


# ---------------------------------------------------------------------------------------------------------------- resampling
def taps_ac(n_in, f):
    """[f·n_in, n_in] bilinear align_corners=True matrix: output o reads source coordinate o·(n_in − 1)/(f·n_in − 1)."""
    n_out = n_in * f
    Wm = torch.zeros(n_out, n_in, dtype=F64)
    for o in range(n_out):
        s = o * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        i0 = min(int(s), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        Wm[o, i0] += 1 - (s - i0)
        Wm[o, i1] += s - i0
    return Wm


def reach_ac(n_in, f):
    """0/1 [f·n_in, n_in]: the sources within one of an output's coordinate.  It holds the neighbour an fp32 coordinate just under an integer
    picks instead, whose weight error multiplies a value that |taps_ac| leaves out."""
    n_out = n_in * f
    s = torch.arange(n_out, dtype=F64) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    return ((torch.arange(n_in, dtype=F64)[None] - s[:, None]).abs() < 1 + 1e-9).to(F64)


def _aa_cubic(x):
    a = -0.5
    x = abs(x)
    if x < 1:
        return ((a + 2) * x - (a + 3)) * x * x + 1
    if x < 2:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def taps_aa(n_in, n_out):
    """[n_out, n_in] antialiased bicubic matrix (align_corners=False): scale = in/out, support = 2·max(scale, 1), window
    [int(centre − support + ½), int(centre + support + ½)) clipped to the axis, cubic a = −0.5 at (j − centre + ½)/max(scale, 1), normalised."""
    scale = n_in / n_out
    support = 2 * max(scale, 1.0)
    inv = 1 / max(scale, 1.0)
    Wm = torch.zeros(n_out, n_in, dtype=F64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), n_in)
        w = [_aa_cubic((j - c + 0.5) * inv) for j in range(lo, hi)]
        tot = sum(w)
        for j in range(lo, hi):
            Wm[i, j] = w[j - lo] / tot
    return Wm


def _sep(Wy, x, Wx):
    """Wy · x · Wxᵀ over the H, W axes of NHWC x."""
    return torch.einsum("oh,bhwc,pw->bopc", Wy, x, Wx)


def _wmag(Wm, reach):
    return torch.maximum(Wm.abs(), reach)


def upsample_ac(x, f, backward=False):
    """uia_upsample_ac on NHWC: forward [B,H,W,C] -> [B,fH,fW,C]; backward: x is the gradient [B,fH,fW,C] -> [B,H,W,C] (the transpose).
    mag: |x| through max(|W|, reach) on both axes, times (1 + max(H, W)): a tap weight's error grows with the source coordinate."""
    x = x.to(F64)
    H, W = (x.shape[1] // f, x.shape[2] // f) if backward else (x.shape[1], x.shape[2])
    Wy, Wx = taps_ac(H, f), taps_ac(W, f)
    My, Mx = _wmag(Wy, reach_ac(H, f)), _wmag(Wx, reach_ac(W, f))
    if backward:
        Wy, Wx, My, Mx = Wy.T, Wx.T, My.T, Mx.T
    return _sep(Wy, x, Wx), _sep(My, x.abs(), Mx) * (1 + max(H, W))


def resize_aa(x, size):
    """uia_resize_aa forward: NHWC x [B,Hi,Wi,C] -> NCHW [B,C,Ho,Wo]; mag: |x| through |W| on both axes, times (1 + the largest of the four
    extents)."""
    x = x.to(F64)
    Hi, Wi = x.shape[1], x.shape[2]
    Ho, Wo = size
    Wy, Wx = taps_aa(Hi, Ho), taps_aa(Wi, Wo)
    ref = _sep(Wy, x, Wx).permute(0, 3, 1, 2)
    mag = _sep(Wy.abs(), x.abs(), Wx.abs()).permute(0, 3, 1, 2)
    return ref, mag * (1 + max(Hi, Wi, Ho, Wo))


def resize_aa_bwd(dout, in_hw):
    """uia_resize_aa backward: NCHW dout [B,C,Ho,Wo] -> NHWC dx [B,Hi,Wi,C], the transpose of resize_aa."""
    g = dout.to(F64).permute(0, 2, 3, 1)
    Hi, Wi = in_hw
    Ho, Wo = g.shape[1], g.shape[2]
    Wy, Wx = taps_aa(Hi, Ho), taps_aa(Wi, Wo)
    ref = _sep(Wy.T, g, Wx.T)
    mag = _sep(Wy.abs().T, g.abs(), Wx.abs().T)
    return ref, mag * (1 + max(Hi, Wi, Ho, Wo))


# ---------------------------------------------------------------------------------------------------------------- the cases both tests run
# (B, H, W, C1, C2, N).  MFMA path: channels % 32 == 0 and N % 4 == 0; 13×11 gives M = 143, one full 128-pixel tile and a 15-pixel tail; the
# last MFMA case has M = 429 and N = 8 for the weight gradient.  Direct path: the rest; (2,3,7,34,30,32) is the data gradient of 32 channels
# into n = 64 split at n1 = 34 (direct, two outputs), (1,7,3,32,64,32) and (1,7,3,64,32,96) the MFMA splits n1 = 32 and 64 of n = 96.
CONV_MFMA = ((2, 3, 7, 32, 0, 32), (1, 7, 3, 64, 32, 96), (2, 1, 9, 32, 32, 64), (2, 9, 1, 32, 0, 36), (1, 13, 11, 32, 0, 64), (1, 1, 1, 32, 0, 4),
             (1, 7, 3, 32, 64, 32), (3, 13, 11, 32, 0, 8))
CONV_DIRECT = ((2, 3, 7, 4, 6, 2), (1, 5, 4, 33, 0, 5), (1, 4, 6, 32, 0, 3), (2, 3, 7, 34, 30, 32))
# (B, h, w, Cin, Cout); the last is the one whose data gradient takes the MFMA path (Cout % 32 == 0)
CONVT = ((2, 3, 5, 32, 4), (1, 5, 3, 64, 24), (2, 2, 3, 32, 3), (1, 1, 1, 32, 8), (1, 4, 2, 6, 5), (1, 3, 2, 32, 32))
BN_C = (1, 3, 96, 200, 256, 257, 384, 520)
BN_M = (2, 255, 256, 257, 1369)
BN_CAP = (66000, 2)         # (M, C): 264·250 rows, past the 256-slice cap (258 rows per slice)
BN_MOMENTA = (0.0, 0.1, 1.0)
UPS_F = (1, 2, 16)
UPS_HW = ((1, 1), (1, 6), (6, 1), (5, 3), (37, 5))
UPS_C = (1, 5)
AA_SIZES = (((12, 20), (9, 8)), ((5, 9), (13, 4)), ((12, 9), (4, 3)), ((1, 11), (1, 7)), ((6, 10), (3, 25)), ((40, 37), (33, 41)), ((7, 5), (7, 5)))
AA_C = (1, 3)


def rnd(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


def bn_case(M, C, dt, seed, mean=3.0):
    """The operands of one BatchNorm case, as the kernel sees them: y [M, C] of dt, fp32 γ, β, running buffers."""
    g = torch.Generator().manual_seed(seed)
    y = (mean + 2.0 * torch.randn(M, C, generator=g)).to(dt)
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    rm, rv = 0.1 * torch.randn(C, generator=g), 1 + 0.1 * torch.rand(C, generator=g)
    return y, gamma, beta, rm, rv


def bn_bwd_case(M, C, dt, seed):
    """The operands of one BatchNorm backward case: y with no element in the ambiguous ReLU band, dout, and the fp32 statistics of y."""
    y, gamma, beta, _, _ = bn_case(M, C, dt, seed, mean=0.5)
    r = bn_train(y, gamma, beta, None, None, None, 0.1, f32(1e-5))
    scale, shift, mean, invstd = (r[k][0].float() for k in ("scale", "shift", "mean", "invstd"))
    y = clear_relu_band(y, scale, shift, dt)
    dout = rnd(M, C, seed=seed + 1).to(dt)
    return y, dout, scale, shift, mean, invstd, gamma
