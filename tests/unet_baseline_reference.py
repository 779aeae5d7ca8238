"""Float64 restatement of the reference's from-scratch UNet baseline (src/third_party/unet.py: UNet(in_channels, num_classes, init_channels)),
on a state dict with the reference's key names, with the dropout masks passed in:

    ConvBlock(x)  = Leaky(BN(Conv3x3(keep/(1−p) · Leaky(BN(Conv3x3(x))))))          Leaky = LeakyReLU(0.01), BN = BatchNorm2d in train / eval mode
    encoder       = in_conv, then four times MaxPool2d(2) -> ConvBlock               dropout p = 0.05, 0.1, 0.2, 0.3, 0.5
    UpBlock(a, s) = ConvBlock(cat[s, Upsample_ac(Conv1x1(a), 2)])                    the branch the reference's Decoder runs; no dropout
    logits        = Conv3x3(up4(up3(up2(up1(x4, x3), x2), x1), x0))

The functions run in the dtype of the state they are given, so the same code gives the float64 reference and the fp32 / bf16 CPU runs that
measure how far plain arithmetic in those formats lands from it.  In bf16 the BatchNorm statistics, buffers and normalisation are fp32 on the
bf16 conv output, as PyTorch's own batch_norm computes them: statistics summed in bf16 would triple the distance (7.8e-2 against 4.5e-2 on the
train logits at c = 16, 48x48) and the bar built on it would mean less.  Also the seeded weights, inputs and keep masks of the small golden geometry
(tools/gen_unet_baseline_golden.py records the reference's outputs on them), and, in the style of tests/unet_reference.py, the element-wise
restatements (ref, mag) of the kernels the baseline added: max-pool, BatchNorm + LeakyReLU + dropout, the 1x1 convolution.
A plain module, no pytest."""
import torch
import torch.nn.functional as F

import unet_reference as UR

F64 = torch.float64
SLOPE = 0.01
DROPOUT = (0.05, 0.1, 0.2, 0.3, 0.5)

# the small golden geometry
SMALL = dict(in_channels=3, num_classes=2, init_channels=8, batch=2, size=32, seed=9753)


def _conv_block_shapes(p, cin, cout):
    out = []
    for i, c_in in ((0, cin), (4, cout)):
        out += [(f"{p}.{i}.weight", (cout, c_in, 3, 3)), (f"{p}.{i}.bias", (cout,)), (f"{p}.{i + 1}.weight", (cout,)), (f"{p}.{i + 1}.bias", (cout,)),
                (f"{p}.{i + 1}.running_mean", (cout,)), (f"{p}.{i + 1}.running_var", (cout,)), (f"{p}.{i + 1}.num_batches_tracked", ())]
    return out


def state_shapes(in_channels, num_classes, init_channels=16):
    """(name, shape) of UNet(in_channels, num_classes, init_channels) in the reference's state-dict order (BatchNorm buffers included)."""
    ch = [init_channels << i for i in range(5)]
    out = _conv_block_shapes("encoder.in_conv.conv_conv", in_channels, ch[0])
    for i in range(1, 5):
        out += _conv_block_shapes(f"encoder.down{i}.maxpool_conv.1.conv_conv", ch[i - 1], ch[i])
    for i in range(1, 5):
        c1, c2 = ch[5 - i], ch[4 - i]
        out += [(f"decoder.up{i}.conv1x1.weight", (c2, c1, 1, 1)), (f"decoder.up{i}.conv1x1.bias", (c2,))]
        out += _conv_block_shapes(f"decoder.up{i}.conv.conv_conv", 2 * c2, c2)
    return out + [("decoder.out_conv.weight", (num_classes, ch[0], 3, 3)), ("decoder.out_conv.bias", (num_classes,))]


def is_buffer(k):
    return "running" in k or "num_batches" in k


def seeded_state(in_channels, num_classes, init_channels, seed):
    """Weights drawn from one CPU generator in key order: convs N(0, 1/fan_in), biases N(0, 0.1²), BN γ = 1 + N(0, 0.1²), β N(0, 0.1²);
    running_mean 0, running_var 1, num_batches_tracked 0 (a fresh module's buffers)."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for k, shp in state_shapes(in_channels, num_classes, init_channels):
        if k.endswith("num_batches_tracked"):
            P[k] = torch.zeros((), dtype=torch.int64)
        elif k.endswith("running_mean"):
            P[k] = torch.zeros(shp, dtype=F64)
        elif k.endswith("running_var"):
            P[k] = torch.ones(shp, dtype=F64)
        elif len(shp) == 1 and k.endswith("weight"):
            P[k] = 1.0 + 0.1 * torch.randn(shp, generator=g, dtype=F64)
        elif k.endswith("bias"):
            P[k] = 0.1 * torch.randn(shp, generator=g, dtype=F64)
        else:
            P[k] = torch.randn(shp, generator=g, dtype=F64) / (shp[1] * shp[2] * shp[3]) ** 0.5
    return P


def seeded_inputs(in_channels, num_classes, batch, size, seed, **_):
    """The image batch [B, C, S, S] and the upstream gradient of the logits [B, num_classes, S, S]."""
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(batch, in_channels, size, size, generator=g, dtype=F64)
    dlogits = torch.randn(batch, num_classes, size, size, generator=g, dtype=F64)
    return x, dlogits


def seeded_masks(init_channels, batch, size, seed, **_):
    """The five keep masks (NCHW float64 of 0 / 1), one per encoder block, kept with probability 1 − p."""
    g = torch.Generator().manual_seed(seed + 2)
    return [(torch.rand(batch, init_channels << i, size >> i, size >> i, generator=g, dtype=F64) >= p).to(F64) for i, p in enumerate(DROPOUT)]


def cast_state(P, dt):
    return {k: (v if v.dtype == torch.int64 else v.to(dt)) for k, v in P.items()}


def _cbl(P, p, i, x, training, bufs):
    """LeakyReLU(BatchNorm2d(Conv3x3)) of conv_conv.{i, i+1}."""
    y = F.conv2d(x, P[f"{p}.{i}.weight"], P[f"{p}.{i}.bias"], padding=1)
    dt = y.dtype
    if dt == torch.bfloat16:
        y = y.float()                  # BatchNorm on a bf16 tensor: statistics, buffers and the normalisation in fp32, as F.batch_norm does
    bn = f"{p}.{i + 1}"
    rm, rv = bufs[bn + ".running_mean"].to(y.dtype), bufs[bn + ".running_var"].to(y.dtype)
    if training:
        n = y.shape[0] * y.shape[2] * y.shape[3]
        mean = y.mean(dim=(0, 2, 3))
        var = y.var(dim=(0, 2, 3), unbiased=False)
        bufs[bn + ".running_mean"] = (0.9 * rm + 0.1 * mean).detach()
        bufs[bn + ".running_var"] = (0.9 * rv + 0.1 * var * n / (n - 1)).detach()
        bufs[bn + ".num_batches_tracked"] = bufs[bn + ".num_batches_tracked"] + 1
    else:
        mean, var = rm, rv
    gamma, beta = P[bn + ".weight"].to(y.dtype), P[bn + ".bias"].to(y.dtype)
    z = (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + 1e-5) * gamma[None, :, None, None] + beta[None, :, None, None]
    return F.leaky_relu(z.to(dt), SLOPE)


def _conv_block(P, p, x, training, bufs, drop_p, mask):
    x = _cbl(P, p, 0, x, training, bufs)
    if training and drop_p > 0:
        x = x * mask.to(x.dtype) / (1 - drop_p)
    return _cbl(P, p, 4, x, training, bufs)


def unet_forward(P, x, masks=None, training=True, bufs=None):
    """UNet on NCHW x in the dtype of P.  masks: the five keep masks (training).  bufs: the BatchNorm buffers (a dict, updated in training;
    default: those of P).  Returns (logits [B, num_classes, H, W], bufs)."""
    bufs = {k: v.clone() for k, v in P.items() if is_buffer(k)} if bufs is None else bufs
    masks = masks if masks is not None else [None] * 5
    if x.shape[1] == 1:
        x = x.expand(-1, 3, -1, -1)
    feats = [_conv_block(P, "encoder.in_conv.conv_conv", x, training, bufs, DROPOUT[0], masks[0])]
    for i in range(1, 5):
        feats.append(_conv_block(P, f"encoder.down{i}.maxpool_conv.1.conv_conv", F.max_pool2d(feats[-1], 2), training, bufs, DROPOUT[i], masks[i]))
    x = feats[4]
    for i in range(1, 5):
        a = F.conv2d(x, P[f"decoder.up{i}.conv1x1.weight"], P[f"decoder.up{i}.conv1x1.bias"])
        a = F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=True)
        x = _conv_block(P, f"decoder.up{i}.conv.conv_conv", torch.cat([feats[4 - i], a], dim=1), training, bufs, 0.0, None)
    return F.conv2d(x, P["decoder.out_conv.weight"], P["decoder.out_conv.bias"], padding=1), bufs


def run_restatement(P64, x, masks, dlogits, dt):
    """The restatement in dtype dt on the CPU: train-mode logits, buffers after that forward, the gradient of every parameter for the upstream
    gradient dlogits, and the eval-mode logits that follow.  Everything is returned in float64."""
    P = cast_state(P64, dt)
    names = [k for k in P if not is_buffer(k)]
    for k in names:
        P[k] = P[k].clone().requires_grad_(True)
    out, bufs = unet_forward(P, x.to(dt), masks, training=True)
    (out * dlogits.to(dt)).sum().backward()
    grads = {k: P[k].grad.to(F64) for k in names}
    with torch.no_grad():
        ev, _ = unet_forward({k: v.detach() for k, v in P.items()}, x.to(dt), None, training=False, bufs=dict(bufs))
    return out.detach().to(F64), {k: (v if v.dtype == torch.int64 else v.to(F64)) for k, v in bufs.items()}, grads, ev.to(F64)


def conv_launches(in_channels=3, num_classes=2, c=16):
    """Every convolution launch of one training step of UNet(in_channels, num_classes, c), as (name, kind, mode, C1, C2, N, N1): kind "igemm"
    (forward or data gradient) or "wgrad"; mode 0 = 3x3, 3 = 1x1.  in_conv.0 has no data gradient (the images need none)."""
    ch = [c << i for i in range(5)]
    out = []

    def conv3(name, c1, c2, n, dgrad=True):
        out.append((name + " forward", "igemm", 0, c1, c2, n, n))
        if dgrad:
            out.append((name + " dgrad", "igemm", 0, n, 0, c1 + c2, c1))
        out.append((name + " wgrad", "wgrad", 0, c1, c2, n, None))

    def block(p, c1, c2, n, dgrad=True):
        conv3(p + ".0", c1, c2, n, dgrad)
        conv3(p + ".4", n, 0, n)
    block("encoder.in_conv", in_channels, 0, ch[0], dgrad=False)
    for i in range(1, 5):
        block(f"encoder.down{i}", ch[i - 1], 0, ch[i])
    for i in range(1, 5):
        c1, c2 = ch[5 - i], ch[4 - i]
        name = f"decoder.up{i}.conv1x1"
        out += [(name + " forward", "igemm", 3, c1, 0, c2, c2), (name + " dgrad", "igemm", 3, c2, 0, c1, c1), (name + " wgrad", "wgrad", 3, c1, 0, c2, None)]
        block(f"decoder.up{i}.conv", c2, c2, c2)
    conv3("decoder.out_conv", ch[0], 0, num_classes)
    return out


# ====================================================================================================================================
# Per-kernel restatements, as in tests/unet_reference.py: CPU tensors holding the operands the kernel sees -> (ref, mag) in float64.
# ====================================================================================================================================
def maxpool2(x):
    """uia_maxpool2_fwd on NHWC x: (y [B, H//2, W//2, C], arg) with arg the window position (2·di + dj) of the first maximum."""
    x = x.to(F64)
    Ho, Wo = x.shape[1] // 2, x.shape[2] // 2
    win = [x[:, di:2 * Ho:2, dj:2 * Wo:2] for di in (0, 1) for dj in (0, 1)]
    best, arg = win[0].clone(), torch.zeros(win[0].shape, dtype=torch.int64)
    for t in range(1, 4):
        upd = win[t] > best
        best = torch.where(upd, win[t], best)
        arg = torch.where(upd, torch.full_like(arg, t), arg)
    return best, arg


def maxpool2_bwd(x, dy):
    """uia_maxpool2_bwd: dx [B, H, W, C], dy at each window's first maximum, zero elsewhere and in a trailing odd row / column."""
    _, arg = maxpool2(x)
    dy = dy.to(F64)
    Ho, Wo = dy.shape[1], dy.shape[2]
    dx = torch.zeros(x.shape, dtype=F64)
    for t in range(4):
        dx[:, t >> 1:2 * Ho:2, t & 1:2 * Wo:2] = torch.where(arg == t, dy, torch.zeros_like(dy))
    return dx


C_ACT = 3          # on top of the BatchNorm constants: one fp32 rounding each for the slope product, 1/(1 − p) and the product with it


def _inv_keep(p):
    return 1.0 / (1.0 - UR.f32(p)) if p > 0 else 1.0


def bn_act_train(y, gamma, beta, run_mean, run_var, nbt, momentum, eps, slope, p, keep):
    """uia_bn_act_fwd in training on rows y [M, C]: UR.bn_train's dict with out = leaky(z)·keep/(1 − p) (keep: 0 / 1 rows, None without
    dropout); its magnitude is that of z times 1/(1 − p) (|slope·z| ≤ |z|)."""
    r = UR.bn_train(y, gamma, beta, run_mean, run_var, nbt, momentum, eps, relu=False)
    z, mag = r["out"]
    k = _inv_keep(p) * (keep.to(F64) if keep is not None and p > 0 else 1.0)
    r["out"] = (F.leaky_relu(z, slope) * k, mag * _inv_keep(p))
    return r


def bn_act_eval(y, gamma, beta, run_mean, run_var, eps, slope):
    """uia_bn_act_fwd in eval mode: running statistics, no dropout."""
    z, mag = UR.bn_eval(y, gamma, beta, run_mean, run_var, eps, relu=False)
    return F.leaky_relu(z, slope), mag


def bn_act_bwd(y, dout, scale, shift, mean, invstd, gamma, slope, p, keep):
    """uia_bn_act_bwd on rows [M, C] from the saved fp32 statistics: dz = dout·keep/(1 − p)·(z > 0 ? 1 : slope) (z == 0 takes the slope), then
    UR.bn_relu_bwd's formulas.  Returns its dict (dy, dgamma, dbeta as (ref, mag); z, band)."""
    y, dout, scale, shift, mean, invstd, gamma = (t.to(F64) for t in (y, dout, scale, shift, mean, invstd, gamma))
    M = y.shape[0]
    g = dout * _inv_keep(p) * (keep.to(F64) if keep is not None and p > 0 else 1.0)
    z = y * scale + shift
    dz = torch.where(z > 0, g, slope * g)
    xh = (y - mean) * invstd
    dbeta, dgamma = dz.sum(0), (dz * xh).sum(0)
    mag_db, mag_dg = dz.abs().sum(0), (dz * xh).abs().sum(0)
    k = (gamma * invstd).abs()
    dy = gamma * invstd * (dz - dbeta / M - xh * dgamma / M)
    mag_dy = k * (dz.abs() + (mag_db + dbeta.abs()) / M + xh.abs() * (mag_dg + dgamma.abs()) / M)
    return dict(dy=(dy, mag_dy), dgamma=(dgamma, mag_dg), dbeta=(dbeta, mag_db), z=z.abs(), band=2 * 2.0 ** -24 * ((y * scale).abs() + shift.abs()))


def conv1x1(x, w, bias=None):
    """UIA_CONV1: x [B,H,W,C1], w [N, C1], bias [N] -> [B,H,W,N].  The data gradient is conv1x1(dy, wᵀ)."""
    x, w = x.to(F64), w.to(F64)
    ref, mag = x @ w.T, x.abs() @ w.abs().T
    return (ref, mag) if bias is None else (ref + bias.to(F64), mag + bias.to(F64).abs())


def conv1x1_wgrad(x, dy):
    """dW[n, c] = Σ_{b,y,x} dy[b, y, x, n]·x[b, y, x, c]."""
    x, g = x.to(F64), dy.to(F64)
    return torch.einsum("bhwn,bhwc->nc", g, x), torch.einsum("bhwn,bhwc->nc", g.abs(), x.abs())


# ---------------------------------------------------------------------------------------------------------------- the cases
POOL = ((1, 2, 2, 1), (1, 2, 2, 8), (2, 4, 6, 24), (1, 5, 7, 3), (1, 3, 2, 16), (3, 8, 8, 40), (1, 6, 4, 12))      # (B, H, W, C)
POOL_DATA = ("random", "negative", "equal", "binary")
# (B, H, W, C1, C2, N): channel counts multiples of 8 that are not multiples of 32 (the generalised MFMA kernel), K = 9·Cin no multiple of 32
# (zero-filled last step: 72, 144, 216, 360), a second source, N past one 16-row fragment, a 143-pixel grid (one full tile and a tail)
CONV3_CASES = ((1, 1, 1, 8, 0, 4), (2, 3, 7, 16, 0, 16), (1, 7, 3, 16, 16, 16), (1, 5, 4, 8, 24, 12), (1, 13, 11, 16, 0, 64), (1, 4, 6, 40, 0, 8),
               (2, 3, 5, 48, 16, 20))
# weight-gradient split counts: M = 4096 pixels -> 128 ranges of 32, M = 18432 -> the cap of 512 (three tiles, 8 workgroups per CU wanted)
WGRAD_SPLIT_CASES = ((1, 64, 64, 8, 24, 16), (2, 96, 96, 16, 0, 16))
CONV1_CASES = ((2, 3, 5, 32, 0, 16), (1, 1, 1, 16, 0, 8), (1, 4, 4, 24, 0, 8), (1, 3, 3, 3, 0, 2))
CONVT_CASES = ((2, 3, 5, 16, 8), (1, 2, 3, 8, 16))                       # (B, h, w, Cin, Cout)
DROP_P = (0.0, 0.05, 0.5)


def pool_data(kind, shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        x = torch.randn(*shape, generator=g)
    elif kind == "negative":
        x = -0.5 - torch.rand(*shape, generator=g)
    elif kind == "equal":
        x = torch.full(shape, -1.25)
    else:
        x = torch.randint(0, 2, shape, generator=g).float()
    return x.to(dt)


def keep_rows(M, C, p, seed):
    """A uint8 keep mask [M, C] with keep probability 1 − p."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(M, C, generator=g) >= p).to(torch.uint8)
