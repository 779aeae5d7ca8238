"""Float64 restatement of the reference's DINOv2 classifier forward (src/third_party/dino/vision_transformer.py `vit_base` +
DINOV2Encoder(n_last_blocks=4) + ClassificationHead(layers=4), dinov2.py:11-100), on a state dict with the reference's key names.

    tokens  = cat(cls, conv_p(x)) + pos                              (pos_embed as is: the reference never interpolates at its own size)
    block   = x + attn(LN1 x);  x + fc2(gelu_erf(fc1(LN2 x)))        (LayerScale absent: init_values=None, ls*.gamma dropped by strict=False)
    attn    = softmax(q kᵀ / sqrt(64)) v per head                     (MemEffAttention without xFormers)
    feats   = cat[LN(cls_8), LN(cls_9), LN(cls_10), LN(cls_11), mean_l LN(x_11)[1:]]   (the final norm, eps 1e-6)
    logits  = feats · Wᵀ + b

Also the seeded weights of the small golden geometry (tools/gen_dino_golden.py records the reference's outputs on them): seeded_state() draws every
tensor from one CPU generator in key order, so the test regenerates the same weights instead of storing them.
A plain module, no pytest: tests/test_dino_host.py checks it against tests/golden/dino_small.npz, tests/test_dino_gpu.py runs the kernels against it."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
EPS = 1e-6

# the small golden geometry: head dim 64, four blocks, 336 px at patch 14 -> 24 x 24 patches + CLS = 577 tokens (past the single-pass 272)
SMALL = dict(img_size=336, patch_size=14, embed_dim=128, depth=4, num_heads=2, num_classes=3, batch=2, seed=1234)


def state_shapes(img_size, patch_size, embed_dim, depth, num_classes, mlp_ratio=4):
    """(name, shape) in the reference's state-dict order (encoder.* of DINOV2Encoder, then linear.* of ClassificationHead(layers=4))."""
    D, F_ = embed_dim, int(embed_dim * mlp_ratio)
    n = (img_size // patch_size) ** 2
    out = [("encoder.cls_token", (1, 1, D)), ("encoder.pos_embed", (1, n + 1, D)), ("encoder.mask_token", (1, D)),
           ("encoder.patch_embed.proj.weight", (D, 3, patch_size, patch_size)), ("encoder.patch_embed.proj.bias", (D,))]
    for i in range(depth):
        p = f"encoder.blocks.0.{i}."
        out += [(p + "norm1.weight", (D,)), (p + "norm1.bias", (D,)), (p + "attn.qkv.weight", (3 * D, D)), (p + "attn.qkv.bias", (3 * D,)),
                (p + "attn.proj.weight", (D, D)), (p + "attn.proj.bias", (D,)), (p + "norm2.weight", (D,)), (p + "norm2.bias", (D,)),
                (p + "mlp.fc1.weight", (F_, D)), (p + "mlp.fc1.bias", (F_,)), (p + "mlp.fc2.weight", (D, F_)), (p + "mlp.fc2.bias", (D,))]
    out += [("encoder.norm.weight", (D,)), ("encoder.norm.bias", (D,)), ("linear.weight", (num_classes, 5 * D)), ("linear.bias", (num_classes,))]
    return out


def seeded_state(img_size, patch_size, embed_dim, depth, num_classes, seed):
    """fp32 weights of an informative scale: LayerNorm weights 1 + 0.1·N, biases 0.02·N, matrices N/sqrt(fan_in), embeddings 0.5·N."""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for name, shape in state_shapes(img_size, patch_size, embed_dim, depth, num_classes):
        r = torch.randn(shape, generator=g)
        if "norm" in name and name.endswith("weight"):
            t = 1.0 + 0.1 * r
        elif name.endswith("bias"):
            t = 0.02 * r
        elif name.endswith("weight"):
            fan_in = math.prod(shape[1:])
            t = r / math.sqrt(fan_in)
        else:
            t = 0.5 * r
        state[name] = t.float()
    return state


def seeded_images(batch, img_size, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.rand(batch, 3, img_size, img_size, generator=g)


def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, EPS)


def forward(images, P, num_heads, patch_size, n_last=4, device=None):
    """float64 (features [B, (n_last + 1)·D], logits [B, C]); P: the reference-named state dict (any dtype), images [B, 3, H, W]."""
    dev = device if device is not None else images.device
    P = {k: v.to(dev, F64) for k, v in P.items()}
    x = images.to(dev, F64)
    e = "encoder."
    t = F.conv2d(x, P[e + "patch_embed.proj.weight"], P[e + "patch_embed.proj.bias"], stride=patch_size).flatten(2).transpose(1, 2)
    B, n, D = t.shape
    if n + 1 != P[e + "pos_embed"].shape[1]:
        raise ValueError("image size differs from the one the position embedding was built for")
    t = torch.cat([P[e + "cls_token"].expand(B, 1, D), t], 1) + P[e + "pos_embed"]
    N, dh = n + 1, D // num_heads
    depth = len({k.split(".")[3] for k in P if k.startswith(e + "blocks.0.")})
    outs = []
    for i in range(depth):
        p = f"{e}blocks.0.{i}."
        h = _ln(t, P[p + "norm1.weight"], P[p + "norm1.bias"])
        qkv = (h @ P[p + "attn.qkv.weight"].T + P[p + "attn.qkv.bias"]).reshape(B, N, 3, num_heads, dh).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, -1) @ v
        t = t + a.transpose(1, 2).reshape(B, N, D) @ P[p + "attn.proj.weight"].T + P[p + "attn.proj.bias"]
        h = _ln(t, P[p + "norm2.weight"], P[p + "norm2.bias"])
        h = F.gelu(h @ P[p + "mlp.fc1.weight"].T + P[p + "mlp.fc1.bias"])
        t = t + h @ P[p + "mlp.fc2.weight"].T + P[p + "mlp.fc2.bias"]
        if i >= depth - n_last:
            outs.append(_ln(t, P[e + "norm.weight"], P[e + "norm.bias"]))
    feats = torch.cat([o[:, 0] for o in outs] + [outs[-1][:, 1:].mean(1)], 1)
    logits = feats @ P["linear.weight"].T + P["linear.bias"]
    return feats, logits
