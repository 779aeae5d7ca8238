"""Float64 restatement of the ResNet classification baseline (src/third_party/resnet.py: torchvision's ResNet with BasicBlock, written for
this project from its documented structure), on a state dict with torchvision's key names:

    stem          = MaxPool3/2/1(ReLU(BN(Conv7x7 s2 p3(x))))
    BasicBlock(x) = ReLU(BN(Conv3x3(ReLU(BN(Conv3x3 stride(x))))) + id(x)),  id = x or BN(Conv1x1 stride(x))
    logits        = Linear(mean over the pixels of layer4(layer3(layer2(layer1(stem)))))

The functions run in the dtype of the state they are given, so the same code gives the float64 reference and the bf16 CPU run that measures
how far plain arithmetic in that format lands from it (BatchNorm statistics in fp32 on the bf16 conv output, as in
tests/unet_baseline_reference.py).  Then, in the style of tests/unet_reference.py, the element-wise restatements (ref, mag) of the kernels
the baseline added: the strided convolution (forward, data gradient, weight gradient) written tap by tap on NHWC, the 3/2/1 max-pool,
BatchNorm + add + ReLU, the average pool.  tests/test_resnet_baseline_host.py checks each of them against torch.nn.functional and autograd.
A plain module, no pytest."""
import torch
import torch.nn.functional as F

import unet_reference as UR

F64 = torch.float64
STAGES = (64, 128, 256, 512)
LAYERS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}


# ---------------------------------------------------------------------------------------------------------------- the model
def _bn_shapes(p, c):
    return [(p + ".weight", (c,)), (p + ".bias", (c,)), (p + ".running_mean", (c,)), (p + ".running_var", (c,)), (p + ".num_batches_tracked", ())]


def blocks(version="resnet18"):
    """(prefix, inplanes, planes, stride, has_downsample) of every BasicBlock in order."""
    out, inplanes = [], 64
    for li, (planes, n) in enumerate(zip(STAGES, LAYERS[version]), start=1):
        for i in range(n):
            stride = 2 if (i == 0 and li > 1) else 1
            out.append((f"layer{li}.{i}", inplanes, planes, stride, i == 0 and (stride != 1 or inplanes != planes)))
            inplanes = planes
    return out


def state_shapes(version="resnet18", num_classes=1000):
    """(name, shape) of torchvision's resnet18 / resnet34 state dict, in its order (BatchNorm buffers included)."""
    out = [("conv1.weight", (64, 3, 7, 7))] + _bn_shapes("bn1", 64)
    for p, cin, c, _, ds in blocks(version):
        out += [(p + ".conv1.weight", (c, cin, 3, 3))] + _bn_shapes(p + ".bn1", c) + [(p + ".conv2.weight", (c, c, 3, 3))] + _bn_shapes(p + ".bn2", c)
        if ds:
            out += [(p + ".downsample.0.weight", (c, cin, 1, 1))] + _bn_shapes(p + ".downsample.1", c)
    return out + [("fc.weight", (num_classes, 512)), ("fc.bias", (num_classes,))]


def conv_launches(version="resnet18"):
    """Every convolution of the model as (name, Cin as launched, Cout, k, stride, has_dgrad): the stem with its 3 channels packed in 8 and no
    data gradient.  Each is a forward and a weight-gradient launch, and a data-gradient launch where has_dgrad."""
    out = [("conv1", 8, 64, 7, 2, False)]
    for p, cin, c, stride, ds in blocks(version):
        out += [(p + ".conv1", cin, c, 3, stride, True), (p + ".conv2", c, c, 3, 1, True)]
        if ds:
            out.append((p + ".downsample.0", cin, c, 1, stride, True))
    return out


def is_buffer(k):
    return "running" in k or "num_batches" in k


def seeded_state(version, num_classes, seed):
    """Weights drawn from one CPU generator in key order: convs N(0, 2/fan_in) (He: the activations keep their scale through the ReLUs),
    BN γ = 1 + N(0, 0.1²), β N(0, 0.1²), fc N(0, 1/512) and bias N(0, 0.1²); the buffers of a fresh module."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for k, shp in state_shapes(version, num_classes):
        if k.endswith("num_batches_tracked"):
            P[k] = torch.zeros((), dtype=torch.int64)
        elif k.endswith("running_mean"):
            P[k] = torch.zeros(shp, dtype=F64)
        elif k.endswith("running_var"):
            P[k] = torch.ones(shp, dtype=F64)
        elif len(shp) == 4:
            P[k] = torch.randn(shp, generator=g, dtype=F64) * (2.0 / (shp[1] * shp[2] * shp[3])) ** 0.5
        elif k == "fc.weight":
            P[k] = torch.randn(shp, generator=g, dtype=F64) / shp[1] ** 0.5
        elif k.endswith("bias"):
            P[k] = 0.1 * torch.randn(shp, generator=g, dtype=F64)
        else:
            P[k] = 1.0 + 0.1 * torch.randn(shp, generator=g, dtype=F64)
    return P


def seeded_inputs(batch, size, num_classes, seed, channels=3):
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(batch, channels, size, size, generator=g, dtype=F64)
    dlogits = torch.randn(batch, num_classes, generator=g, dtype=F64)
    return x, dlogits


def cast_state(P, dt):
    return {k: (v if v.dtype == torch.int64 else v.to(dt)) for k, v in P.items()}


def _bn(P, bn, y, training, bufs):
    dt = y.dtype
    if dt == torch.bfloat16:
        y = y.float()                  # statistics, buffers and the normalisation in fp32 on the bf16 conv output, as F.batch_norm does
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
    return z, dt


def resnet_forward(P, x, version="resnet18", training=True, bufs=None):
    """The ResNet on NCHW x in the dtype of P.  bufs: the BatchNorm buffers (a dict, updated in training; default: those of P).  A one-channel
    x is three equal channels.  Returns (logits [B, num_classes], bufs)."""
    bufs = {k: v.clone() for k, v in P.items() if is_buffer(k)} if bufs is None else bufs
    if x.shape[1] == 1:
        x = x.expand(-1, 3, -1, -1)
    z, dt = _bn(P, "bn1", F.conv2d(x, P["conv1.weight"], stride=2, padding=3), training, bufs)
    x = F.max_pool2d(torch.relu(z.to(dt)), 3, 2, 1)
    for p, _, _, stride, ds in blocks(version):
        z, dt = _bn(P, p + ".bn1", F.conv2d(x, P[p + ".conv1.weight"], stride=stride, padding=1), training, bufs)
        h = torch.relu(z.to(dt))
        z, dt = _bn(P, p + ".bn2", F.conv2d(h, P[p + ".conv2.weight"], padding=1), training, bufs)
        if ds:
            r, _ = _bn(P, p + ".downsample.1", F.conv2d(x, P[p + ".downsample.0.weight"], stride=stride), training, bufs)
            r = r.to(dt)
        else:
            r = x
        x = torch.relu((z + r.to(z.dtype)).to(dt))
    pooled = x.float().mean(dim=(2, 3)).to(x.dtype) if x.dtype == torch.bfloat16 else x.mean(dim=(2, 3))
    return F.linear(pooled, P["fc.weight"], P["fc.bias"]), bufs


def run_restatement(P64, x, dlogits, dt, version="resnet18"):
    """The restatement in dtype dt on the CPU: train-mode logits, buffers after that forward, the gradient of every parameter for the upstream
    gradient dlogits, and the eval-mode logits that follow.  Everything is returned in float64."""
    P = cast_state(P64, dt)
    names = [k for k in P if not is_buffer(k)]
    for k in names:
        P[k] = P[k].clone().requires_grad_(True)
    out, bufs = resnet_forward(P, x.to(dt), version, training=True)
    (out * dlogits.to(dt)).sum().backward()
    grads = {k: P[k].grad.to(F64) for k in names}
    with torch.no_grad():
        ev, _ = resnet_forward({k: v.detach() for k, v in P.items()}, x.to(dt), version, training=False, bufs=dict(bufs))
    return out.detach().to(F64), {k: (v if v.dtype == torch.int64 else v.to(F64)) for k, v in bufs.items()}, grads, ev.to(F64)


# ====================================================================================================================================
# Per-kernel restatements, as in tests/unet_reference.py: CPU tensors holding the operands the kernel sees -> (ref, mag) in float64.
# The bounds are that module's: c_conv(k², C) for the forward, c_conv(k², N) for the data gradient, c_wgrad(B·Ho·Wo, splits).
# ====================================================================================================================================
def out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def _tap(xp, ky, kx, Ho, Wo, s):
    """The [B, Ho, Wo, C] view of the padded map that tap (ky, kx) multiplies."""
    return xp[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s]


def _pad(x, h):
    return F.pad(x, (0, 0, h, h, h, h))


def conv_strided(x, w, k, s):
    """uia_conv_strided forward: x [B,H,W,C], w [N, k²·C] (column (ky·k + kx)·C + c) -> [B,Ho,Wo,N]."""
    x, w = x.to(F64), w.to(F64)
    B, H, W, C = x.shape
    N = w.shape[0]
    Ho, Wo = out_hw(H, W, s)
    wt = w.reshape(N, k * k, C)

    def run(xx, ww):
        xp = _pad(xx, k // 2)
        out = torch.zeros(B, Ho, Wo, N, dtype=F64)
        for t in range(k * k):
            out = out + _tap(xp, t // k, t % k, Ho, Wo, s) @ ww[:, t].T
        return out
    return run(x, wt), run(x.abs(), wt.abs())


def dgrad_rows(w, k, C):
    """The rows the data gradient takes, [C, k²·N] (column tap·N + n), from the forward rows w [N, k²·C]."""
    N = w.shape[0]
    return w.reshape(N, k * k, C).permute(2, 1, 0).reshape(C, k * k * N).contiguous()


def conv_strided_dgrad(dy, wd, in_hw, k, s):
    """uia_conv_strided data gradient: dy [B,Ho,Wo,N], wd [C, k²·N] -> dx [B,H,W,C]: every output pixel scatters through tap (ky, kx) to
    input pixel (s·y + ky − k/2, s·x + kx − k/2) — the transpose of the forward's gather."""
    dy, wd = dy.to(F64), wd.to(F64)
    B, Ho, Wo, N = dy.shape
    H, W = in_hw
    C = wd.shape[0]
    h = k // 2
    wt = wd.reshape(C, k * k, N)

    def run(g, ww):
        dxp = torch.zeros(B, H + 2 * h, W + 2 * h, C, dtype=F64)
        for t in range(k * k):
            _tap(dxp, t // k, t % k, Ho, Wo, s).add_(g @ ww[:, t].T)
        return dxp[:, h:h + H, h:h + W].contiguous()
    return run(dy, wt), run(dy.abs(), wt.abs())


def conv_strided_wgrad(x, dy, k, s):
    """dW[n, tap·C + c] = Σ_{b,y,x} dy[b, y, x, n]·x[b, s·y + ky − k/2, s·x + kx − k/2, c]."""
    x, g = x.to(F64), dy.to(F64)
    Ho, Wo, N, C = g.shape[1], g.shape[2], g.shape[3], x.shape[3]

    def run(xx, gg):
        xp = _pad(xx, k // 2)
        return torch.stack([torch.einsum("bhwn,bhwc->nc", gg, _tap(xp, t // k, t % k, Ho, Wo, s)) for t in range(k * k)], dim=1).reshape(N, k * k * C)
    return run(x, g), run(x.abs(), g.abs())


def _windows(x):
    """The nine [B, Ho, Wo, C] views of MaxPool2d(3, 2, 1)'s windows over x padded with −inf, in row-major window order."""
    B, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, 2)
    xp = torch.full((B, H + 2, W + 2, C), float("-inf"), dtype=F64)
    xp[:, 1:H + 1, 1:W + 1] = x
    return [_tap(xp, t // 3, t % 3, Ho, Wo, 2) for t in range(9)]


def maxpool3s2(x):
    """uia_maxpool3s2_fwd on NHWC x: (y, arg) with arg the window position (3·dy + dx) of the first maximum."""
    win = _windows(x.to(F64))
    best, arg = win[0].clone(), torch.zeros(win[0].shape, dtype=torch.int64)
    for t in range(1, 9):
        upd = win[t] > best
        best = torch.where(upd, win[t], best)
        arg = torch.where(upd, torch.full_like(arg, t), arg)
    return best, arg


def maxpool3s2_bwd(x, dy, acc=F64):
    """uia_maxpool3s2_bwd: dx [B,H,W,C], every window's dy added at its first maximum.  An input pixel meets the windows that cover it in
    row-major window order, which is descending tap order; with acc = torch.float32 the sums are the kernel's own, bit for bit (it adds
    in fp32 from 0 and rounds once to the tensor's dtype)."""
    _, arg = maxpool3s2(x)
    dy = dy.to(acc)
    B, H, W, C = x.shape
    Ho, Wo = dy.shape[1], dy.shape[2]
    dxp = torch.zeros(B, H + 2, W + 2, C, dtype=acc)
    for t in reversed(range(9)):
        _tap(dxp, t // 3, t % 3, Ho, Wo, 2).add_(torch.where(arg == t, dy, torch.zeros_like(dy)))
    return dxp[:, 1:H + 1, 1:W + 1].contiguous()


def bn_add_relu_train(y, r, gamma, beta, run_mean, run_var, nbt, momentum, eps):
    """uia_bn_add_relu_fwd in training on rows y, r [M, C]: UR.bn_train's dict with out = relu(z + r) (r None: relu(z)); mag adds |r|."""
    d = UR.bn_train(y, gamma, beta, run_mean, run_var, nbt, momentum, eps, relu=False)
    z, mag = d["out"]
    if r is not None:
        z, mag = z + r.to(F64), mag + r.to(F64).abs()
    d["out"] = (torch.relu(z), mag)
    d["pre"] = z
    return d


def bn_add_relu_eval(y, r, gamma, beta, run_mean, run_var, eps):
    z, mag = UR.bn_eval(y, gamma, beta, run_mean, run_var, eps, relu=False)
    if r is not None:
        z, mag = z + r.to(F64), mag + r.to(F64).abs()
    return torch.relu(z), mag


def bn_add_relu_bwd(y, out, dout, mean, invstd, gamma):
    """uia_bn_add_relu_bwd on rows [M, C] from the forward's out and the saved fp32 statistics: dz = dout·[out > 0] (out == 0 takes 0),
    dr = dz, then UR.bn_relu_bwd's formulas on dz.  Returns dict(dy, dgamma, dbeta: (ref, mag); dr: exact)."""
    y, out, dout, mean, invstd, gamma = (t.to(F64) for t in (y, out, dout, mean, invstd, gamma))
    M = y.shape[0]
    dz = torch.where(out > 0, dout, torch.zeros_like(dout))
    xh = (y - mean) * invstd
    dbeta, dgamma = dz.sum(0), (dz * xh).sum(0)
    mag_db, mag_dg = dz.abs().sum(0), (dz * xh).abs().sum(0)
    k = (gamma * invstd).abs()
    dy = gamma * invstd * (dz - dbeta / M - xh * dgamma / M)
    mag_dy = k * (dz.abs() + (mag_db + dbeta.abs()) / M + xh.abs() * (mag_dg + dgamma.abs()) / M)
    return dict(dy=(dy, mag_dy), dgamma=(dgamma, mag_dg), dbeta=(dbeta, mag_db), dr=dz)


C_ADD = 1            # on top of the BatchNorm constants: the fp32 addition of r


def c_avgpool(hw):
    """uia_avgpool_fwd: the H·W pixels added one after another, and the division."""
    return hw + 1


def avgpool(x):
    """uia_avgpool_fwd: NHWC x -> [B, C], (ref, mag)."""
    x = x.to(F64)
    return x.mean(dim=(1, 2)), x.abs().mean(dim=(1, 2))


def avgpool_bwd(dout, hw):
    """uia_avgpool_bwd: dout [B, C] -> dx [B, H, W, C] = dout/(H·W), (ref, mag); one fp32 division."""
    H, W = hw
    d = (dout.to(F64) / (H * W))[:, None, None, :].expand(-1, H, W, -1).contiguous()
    return d, d.abs()


def pack_image(x, dt):
    """uia_nchw_to_nhwc of the stem: fp32 NCHW [B, 1 or 3, H, W] -> NHWC [B, H, W, 8] of dt, channels 3..7 zero."""
    B, C, H, W = x.shape
    out = torch.zeros(B, H, W, 8, dtype=dt)
    out[..., :3] = x.float().permute(0, 2, 3, 1).expand(-1, -1, -1, 3).to(dt)
    return out


# ---------------------------------------------------------------------------------------------------------------- the cases
KS = tuple((k, s) for k in (1, 3, 7) for s in (1, 2))
GRIDS = ((7, 10), (8, 8), (5, 6))                 # B = 2: 140 pixels (past one 128-pixel tile at stride 1), 128, 60; odd and even sides
CONV_CN = ((8, 8), (32, 64), (40, 72))            # (C, N) on the matrix-core path: N = 72 crosses one 64-row tile, C = 40 is no multiple of 32
CONV_DIRECT_CN = ((3, 2),)
POOL_HW = ((7, 9), (8, 8), (2, 3))
POOL_C = (8, 20)
POOL_DATA = ("random", "equal", "negative", "ties")
BN_M = (49, 128, 257)                             # 1·7·7 and 2·8·8; 257: two slices, the last one shorter
BN_C = (8, 64, 20, 257)                           # 257: one row lane per channel and a second pass over the channels
AVG_HW = ((1, 1), (7, 7))
AVG_C = (8, 20, 512)


def pool_data(kind, shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        x = torch.randn(*shape, generator=g)
    elif kind == "negative":
        x = -0.5 - torch.rand(*shape, generator=g)
    elif kind == "equal":
        x = torch.full(shape, -1.25)
    else:
        x = torch.randint(0, 3, shape, generator=g).float() - 1.0
    return x.to(dt)
