"""Times the ResNet baseline with HIP events.  Prints one JSON line.

  (a) --part step: the whole training step (forward, focal loss, backward, optimizer) at B = 32, 224 px, bf16, median ms of 20 after 5 warm-up
      runs: the HIP ResNet-18 through engine.segmentation_step, and as a yardstick the same ResNet-18 as eager PyTorch-ROCm modules (MIOpen
      convs, torch BatchNorm / ReLU / MaxPool2d / AdaptiveAvgPool2d / Linear) in bf16 NCHW with torch.optim.AdamW, in the same run.  Forward and
      forward + backward are reported apart.
  (b) --part convs: the three strided 3x3 shapes of ResNet-18 at that batch ((B,56,56,64)->128, (B,28,28,128)->256, (B,14,14,256)->512, stride 2)
      and the packed stem ((B,224,224,8)->64, 7x7 stride 2): forward, weight gradient and (not for the stem) data gradient, on the matrix-core
      kernel and on the direct kernel (the same call with its operands one element into their buffers, which the dispatch sends to the
      direct form), each measured five times: the median of the five and their spread (min .. max).

    python tools/time_resnet_baseline.py [--part step|convs|all] [--batch 32] [--size 224]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd")]

# (H, W, C, N, k, s, has_dgrad) at 224 px
CONV_SHAPES = ((56, 56, 64, 128, 3, 2, True), (28, 28, 128, 256, 3, 2, True), (14, 14, 256, 512, 3, 2, True), (224, 224, 8, 64, 7, 2, False))


def median_ms(fn, steps=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


class EagerBlock(nn.Module):
    def __init__(self, cin, c, stride):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, c, 3, stride, 1, bias=False), nn.BatchNorm2d(c)
        self.conv2, self.bn2 = nn.Conv2d(c, c, 3, 1, 1, bias=False), nn.BatchNorm2d(c)
        self.downsample = nn.Sequential(nn.Conv2d(cin, c, 1, stride, bias=False), nn.BatchNorm2d(c)) if (stride != 1 or cin != c) else None

    def forward(self, x):
        h = self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x)))))
        return F.relu(h + (x if self.downsample is None else self.downsample(x)))


class EagerResNet18(nn.Module):
    """The same network from stock modules: the yardstick, not the product."""

    def __init__(self, nc):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
        blocks, cin = [], 64
        for c, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
            blocks += [EagerBlock(cin, c, stride), EagerBlock(c, c, 1)]
            cin = c
        self.layers = nn.Sequential(*blocks)
        self.fc = nn.Linear(512, nc)

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        return self.fc(self.layers(x).mean(dim=(2, 3)))


def time_step(B, size):
    from src.losses.focal import FocalLoss
    from src.third_party.resnet import resnet18
    from uia_hip import functional as UF
    from uia_hip.engine import FlatAdapterOptimizer, segmentation_step
    UF.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(1)
    x = torch.rand(B, 3, size, size, device="cuda")
    labels = torch.randint(0, 2, (B,), device="cuda")
    crit = FocalLoss(to_onehot_y=True)
    net = resnet18(num_classes=2).cuda().train()
    opt = FlatAdapterOptimizer(list(net.named_parameters()), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.01, max_norm=0.0)
    res = {"hip_step_ms": median_ms(lambda: segmentation_step(net, crit, opt, x, labels))}
    g = torch.randn(B, 2, device="cuda")

    def hip_fwd_bwd():
        net.zero_grad(set_to_none=True)
        net(x).backward(g)
    res["hip_fwd_ms"] = median_ms(lambda: net(x))
    res["hip_fwd_bwd_ms"] = median_ms(hip_fwd_bwd)

    eager = EagerResNet18(2).cuda().to(torch.bfloat16).train()
    eopt = torch.optim.AdamW(eager.parameters(), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.01)
    xb = x.to(torch.bfloat16)

    def eager_step():
        eopt.zero_grad(set_to_none=True)
        crit(eager(xb).float(), labels).backward()
        eopt.step()

    def eager_fwd_bwd():
        eager.zero_grad(set_to_none=True)
        eager(xb).float().backward(g)
    res["eager_step_ms"] = median_ms(eager_step)
    res["eager_fwd_ms"] = median_ms(lambda: eager(xb))
    res["eager_fwd_bwd_ms"] = median_ms(eager_fwd_bwd)
    return res


def off_by_one(t):
    """The same values one element into a buffer: not 16-byte aligned, so the dispatch takes the direct kernel."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def time_convs(B, scale):
    from uia_hip import ops
    dt = torch.bfloat16
    out = {}
    for H, W, C, N, k, s, has_dgrad in CONV_SHAPES:
        H, W = max(1, H * scale // 224), max(1, W * scale // 224)
        Ho, Wo = ops.strided_out_hw(H, W, s)
        g = torch.Generator(device="cuda").manual_seed(H + C + N)
        x = torch.randn(B, H, W, C, device="cuda", generator=g).to(dt)
        dy = torch.randn(B, Ho, Wo, N, device="cuda", generator=g).to(dt)
        w = (torch.randn(N, k * k * C, device="cuda", generator=g) / (k * k * C) ** 0.5).to(dt)
        wb = (torch.randn(C, k * k * N, device="cuda", generator=g) / (k * k * N) ** 0.5).to(dt)
        rec = {}
        for form, (xx, dd, ww, wwb) in (("mfma", (x, dy, w, wb)), ("direct", tuple(off_by_one(t) for t in (x, dy, w, wb)))):
            fns = {"fwd": lambda: ops.conv_strided(xx, ww, N, k, s), "wgrad": lambda: ops.conv_strided_wgrad(xx, dd, k, s)}
            if has_dgrad:
                fns["dgrad"] = lambda: ops.conv_strided_dgrad(dd, wwb, (H, W), C, k, s)
            for name, fn in fns.items():
                five = sorted(median_ms(fn, steps=10, warmup=3) for _ in range(5))
                rec[f"{name}_{form}"] = {"median_ms": round(five[2], 4), "min_ms": round(five[0], 4), "max_ms": round(five[4], 4)}
        out[f"{B}x{H}x{W}x{C}->{N} k{k}s{s}"] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["step", "convs", "all"], default="all")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    args = ap.parse_args()
    res = {"batch": args.batch, "size": args.size, "device": torch.cuda.get_device_name(0)}
    if args.part in ("convs", "all"):
        res["convs"] = time_convs(args.batch, args.size)
    if args.part in ("step", "all"):
        res.update({k: round(v, 3) for k, v in time_step(args.batch, args.size).items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
