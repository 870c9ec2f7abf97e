#!/usr/bin/env python3
"""ResNet-18 / ResNet-50 inference at 224 x 224 on one MI355X (cpu_vision_amd.resnet: one launch per conv + norm [+ add] + ReLU)
against two baselines that share none of the new code, on the same GPU, fp32, eval:

  (a) torch   the torch.nn network with the same parameters (nn.Conv2d / nn.BatchNorm2d / ... forward);
  (b) unfused the same network from the library's earlier public pieces: F.conv2d_bias_act per conv, then torch's batch_norm,
              add and relu on the device; torch's max_pool2d and the library's avg-pool and linear.  (a) - ours is what the
              kernels buy over the vendor library, (b) - ours what fusing the epilogue buys.

Times are HIP events, the median over 7 rounds of `--iters` forwards after a warm-up, the three sides taking turns round by round.
Then the per-layer breakdown of ours: every fused launch timed alone, the slowest `--top` printed with their share of the roofs
(fp32 MFMA 157.3 TFLOP/s, HBM 8 TB/s; algorithmic flops and bytes: x, weights, residual and y once).

  python tools/perf_resnet.py [--models resnet18 resnet50] [--batches 1 64] [--iters 3] [--top 8]
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd import resnet as R  # noqa: E402
from tools.perf_detect import alternate  # noqa: E402

MFMA_TFLOPS, HBM_GBS = 157.3, 8000.0


class _TorchBlock(nn.Module):
    """The reference's block forward over the containers of a library block (baseline a)."""

    def __init__(self, blk):
        super().__init__()
        self.b = blk

    def forward(self, x):
        b = self.b
        identity = x if b.downsample is None else b.downsample[1](b.downsample[0](x))
        out = torch.relu(b.bn1(b.conv1(x)))
        if hasattr(b, "conv3"):
            out = torch.relu(b.bn2(b.conv2(out)))
            out = b.bn3(b.conv3(out))
        else:
            out = b.bn2(b.conv2(out))
        return torch.relu(out + identity)


def torch_forward(net, x):
    with torch.no_grad():
        x = net.maxpool(torch.relu(net.bn1(net.conv1(x))))
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            for blk in layer:
                x = _TorchBlock(blk)(x)
        return net.fc(torch.flatten(net.avgpool(x), 1))


def _unfused(x, conv, bn, relu, residual=None):
    y = F.conv2d_bias_act(x, conv.weight, None, stride=conv.stride, padding=conv.padding, dilation=conv.dilation, groups=conv.groups)
    y = torch.nn.functional.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    if residual is not None:
        y = y + residual
    return torch.relu(y) if relu else y


def unfused_forward(net, x):
    with torch.no_grad():
        x = torch.nn.functional.max_pool2d(_unfused(x, net.conv1, net.bn1, True), 3, 2, 1)
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            for b in layer:
                identity = x if b.downsample is None else _unfused(x, b.downsample[0], b.downsample[1], False)
                out = _unfused(x, b.conv1, b.bn1, True)
                if hasattr(b, "conv3"):
                    out = _unfused(out, b.conv2, b.bn2, True)
                    x = _unfused(out, b.conv3, b.bn3, True, identity)
                else:
                    x = _unfused(out, b.conv2, b.bn2, True, identity)
        x = torch.flatten(F.adaptive_avg_pool2d(x, (1, 1)), 1)
        return F.linear_bias_relu(x, net.fc.weight, net.fc.bias, relu=False)


def layer_rows(net, x, iters):
    """(ms, label, TFLOP/s, GB/s) of every fused launch of one forward, each timed alone on its recorded inputs."""
    calls, orig = [], R.fused_conv_norm

    def spy(xx, conv, norm, cache, relu, residual=None):
        y = orig(xx, conv, norm, cache, relu, residual)
        calls.append((xx, conv, norm, cache, relu, residual, y))
        return y
    R.fused_conv_norm = spy
    try:
        net(x)
    finally:
        R.fused_conv_norm = orig
    rows = []
    for xx, conv, norm, cache, relu, residual, y in calls:
        ms = alternate([lambda: orig(xx, conv, norm, cache, relu, residual)], iters)[0]
        k = conv.kernel_size[0]
        flop = 2.0 * y.numel() * (conv.in_channels // conv.groups) * k * k
        nbytes = 4.0 * (xx.numel() + y.numel() + conv.weight.numel() + (0 if residual is None else residual.numel()))
        label = (f"{k}x{k} s{conv.stride[0]} d{conv.dilation[0]} {conv.in_channels:4d}->{conv.out_channels:4d} @{y.shape[-2]:3d}x{y.shape[-1]:<3d}"
                 f"{' +res' if residual is not None else '     '}")
        rows.append((ms, label, flop / ms / 1e9, nbytes / ms / 1e6))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["resnet18", "resnet50"])
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 64])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--top", type=int, default=8)
    a = ap.parse_args()
    for name in a.models:
        torch.manual_seed(0)
        net = getattr(R, name)().cuda()
        for n in a.batches:
            x = torch.rand((n, 3, 224, 224), device="cuda")
            ours, ref, unf = net(x).detach(), torch_forward(net, x), unfused_forward(net, x)
            scale = float(ref.abs().max())
            print(f"{name} batch {n}: max |ours - torch| / max |torch| = {float((ours - ref).abs().max()) / scale:.2e}, "
                  f"unfused {float((unf - ref).abs().max()) / scale:.2e}", flush=True)
            ms, ms_torch, ms_unf = alternate([lambda: net(x), lambda: torch_forward(net, x), lambda: unfused_forward(net, x)], a.iters)
            print(f"{name} batch {n}: ours {ms:8.3f} ms = {n / ms * 1e3:7.0f} img/s | (a) torch {ms_torch:8.3f} ms ({ms_torch / ms:5.2f}x ours) | "
                  f"(b) unfused {ms_unf:8.3f} ms ({ms_unf / ms:5.2f}x ours)", flush=True)
            rows = layer_rows(net, x, a.iters)
            total = sum(r[0] for r in rows)
            print(f"  {len(rows)} fused conv launches, {total:.3f} ms when timed one by one; the slowest {a.top}:", flush=True)
            for ms_l, label, tf, gbs in sorted(rows, reverse=True)[:a.top]:
                print(f"    {label} {ms_l:7.3f} ms ({ms_l / total * 100:4.1f}%)  {tf:6.1f} TFLOP/s ({tf / MFMA_TFLOPS * 100:4.1f}% MFMA)  "
                      f"{gbs:7.1f} GB/s ({gbs / HBM_GBS * 100:4.1f}% HBM)", flush=True)


if __name__ == "__main__":
    main()
