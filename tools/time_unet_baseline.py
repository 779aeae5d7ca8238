"""Times the UNet baseline with HIP events.  Prints one JSON line.

  (a) --part step: the whole training step (forward, DiceCE, backward, optimizer) at B = 32, 224 px, bf16, median ms of 20 after 5 warm-up
      runs: the HIP UNet through engine.segmentation_step, and as a yardstick the same UNet as eager PyTorch-ROCm modules (MIOpen convs, torch
      BatchNorm / LeakyReLU / Dropout / MaxPool2d / Upsample, torch.cat) in bf16 NCHW with torch.optim.AdamW.
  (b) --part convs: the three full-resolution convolution shapes (B, H, W, C1, C2, N) of UNet(init_channels=16) at that batch,
      (32,224,224,16,0,16), (32,224,224,16,16,16) and (32,112,112,16,0,32): forward, data gradient and weight gradient medians, each measured
      five times: the median of the five and their spread (min .. max).  Only ops.conv_igemm / ops.conv_wgrad are used, so the same script
      runs on a commit from before the widened MFMA dispatch, where these shapes take the direct kernels.

    python tools/time_unet_baseline.py [--part step|convs|all] [--batch 32] [--size 224]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd")]

CONV_SHAPES = ((32, 224, 224, 16, 0, 16), (32, 224, 224, 16, 16, 16), (32, 112, 112, 16, 0, 32))


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


def eager_block(cin, cout, p):
    return nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.LeakyReLU(), nn.Dropout(p),
                         nn.Conv2d(cout, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.LeakyReLU())


class EagerUNet(nn.Module):
    """The same network from stock modules: the yardstick, not the product."""

    def __init__(self, cin, nc, c=16):
        super().__init__()
        ch = [c << i for i in range(5)]
        drop = [0.05, 0.1, 0.2, 0.3, 0.5]
        self.enc = nn.ModuleList([eager_block(cin if i == 0 else ch[i - 1], ch[i], drop[i]) for i in range(5)])
        self.pool = nn.MaxPool2d(2)
        self.one = nn.ModuleList([nn.Conv2d(ch[4 - i], ch[3 - i], 1) for i in range(4)])
        self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
        self.dec = nn.ModuleList([eager_block(2 * ch[3 - i], ch[3 - i], 0.0) for i in range(4)])
        self.out = nn.Conv2d(ch[0], nc, 3, padding=1)

    def forward(self, x):
        feats = []
        for i, blk in enumerate(self.enc):
            x = blk(x if i == 0 else self.pool(x))
            feats.append(x)
        for i in range(4):
            x = self.dec[i](torch.cat([feats[3 - i], self.up(self.one[i](x))], 1))
        return self.out(x)


def time_step(B, size):
    from src.losses.dice import DiceCELoss
    from src.third_party.unet import UNet
    from uia_hip import functional as UF
    from uia_hip.engine import FlatAdapterOptimizer, segmentation_step
    UF.set_compute_dtype(torch.bfloat16)
    UF.set_dropout_seed(1)
    torch.manual_seed(1)
    x = torch.rand(B, 3, size, size, device="cuda")
    labels = (x[:, :1] > 0.5).long()
    crit = DiceCELoss(smooth_nr=1e-8, smooth_dr=1e-8)
    net = UNet(3, 2).cuda().train()
    opt = FlatAdapterOptimizer(list(net.named_parameters()), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.01, max_norm=0.0)
    res = {"hip_step_ms": median_ms(lambda: segmentation_step(net, crit, opt, x, labels))}

    def hip_fwd_bwd():
        net.zero_grad(set_to_none=True)
        net(x).backward(g)
    g = torch.randn(B, 2, size, size, device="cuda")
    res["hip_fwd_ms"] = median_ms(lambda: net(x))
    res["hip_fwd_bwd_ms"] = median_ms(hip_fwd_bwd)

    eager = EagerUNet(3, 2).cuda().to(torch.bfloat16).train()
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


def time_convs(B):
    from uia_hip import ops
    dt = torch.bfloat16
    out = {}
    for shape in CONV_SHAPES:
        _, H, W, C1, C2, N = shape
        Cin = C1 + C2
        g = torch.Generator(device="cuda").manual_seed(H + Cin + N)
        x1 = torch.randn(B, H, W, C1, device="cuda", generator=g).to(dt)
        x2 = torch.randn(B, H, W, C2, device="cuda", generator=g).to(dt) if C2 else None
        dy = torch.randn(B, H, W, N, device="cuda", generator=g).to(dt)
        w = (torch.randn(N, 9 * Cin, device="cuda", generator=g) / (9 * Cin) ** 0.5).to(dt)
        wb = (torch.randn(Cin, 9 * N, device="cuda", generator=g) / (9 * N) ** 0.5).to(dt)
        bias = torch.zeros(N, device="cuda")
        fns = {"fwd": lambda: ops.conv_igemm(ops.CONV3, x1, x2, w, N, bias=bias),
               "dgrad": lambda: ops.conv_igemm(ops.CONV3, dy, None, wb, Cin, n1=C1),
               "wgrad": lambda: ops.conv_wgrad(ops.CONV3, x1, x2, dy, N)}
        rec = {}
        for name, fn in fns.items():
            five = sorted(median_ms(fn, steps=10, warmup=3) for _ in range(5))
            rec[name] = {"median_ms": round(five[2], 4), "min_ms": round(five[0], 4), "max_ms": round(five[4], 4)}
        out["x".join(str(v) for v in (B,) + shape[1:])] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["step", "convs", "all"], default="all")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    args = ap.parse_args()
    res = {"batch": args.batch, "size": args.size, "device": torch.cuda.get_device_name(0)}
    if args.part in ("convs", "all"):
        res["convs"] = time_convs(args.batch)
    if args.part in ("step", "all"):
        res.update({k: round(v, 3) for k, v in time_step(args.batch, args.size).items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
