"""Float64 restatement of the reference's DINOv2 UNet segmentation decoder (src/third_party/dino/dinov2.py:130-260, UNetDecoder with
resize_image=True), on a state dict with the reference's key names (`up{1..4}.{upconv,conv.0,conv.1,skip_conv.0,skip_conv.1}.*`).

    block(x, skip) = CBR_conv(cat[ConvT2x2(x), Upsample_ac(CBR_skip(skip), a.H / 37)])     CBR = ReLU(BatchNorm2d(Conv2d 3x3 pad 1 + bias))
    decoder        = resize(up4(up3(up2(up1(blk11, blk10), blk9), blk8), blk7))              resize = bicubic, antialias, align_corners=False

BatchNorm: batch mean / biased variance in training (running buffers updated with the unbiased variance, momentum 0.1), running statistics in eval.
The logits have passed through the last block's BatchNorm + ReLU before the resize, as in the reference.

Also the seeded weights and inputs of the small golden geometry (tools/gen_dino_seg_golden.py records the reference's outputs on them).
A plain module, no pytest: tests/test_dino_seg_host.py checks it against tests/golden/dino_seg_small.npz, tests/test_dino_seg_gpu.py runs the kernels
against it."""
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
