"""The fused SSIM loss at the bench shape (32 x 1024^2 x 4, window 11, "same") against the eager float32 torch spelling
of the same loss (five grouped conv2d, the elementwise chain, autograd), forward + backward to the image, both on the
GPU, alternating in one process, timed with device events after warm-up.  Prints per repeat and as medians the
microseconds of each, their ratio, the fused pair's algorithmic bytes over 8 TB/s
  forward   read 2 x 16 B/px, write 3 x 16 B/px (the saved planes)                     (80 B/px)
  backward  read 3 x 16 B/px (saved) + 2 x 16 B/px (images), write 16 B/px             (96 B/px)
and the agreement of the two results at that size.  Per-kernel times: run this tool under rocprofv3 --kernel-trace
--stats.  There is no fallback: without a GPU the tool fails.

    python tools/ssim_bench.py [--batch 32] [--size 1024] [--iters 5] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from pytorch_mesh_renderer_amd.mesh_renderer import losses

PEAK = 8.0e12
BYTES_PER_PIXEL = 80 + 96


def eager_float32_ssim(image, target, window_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """The loss as a user would spell it in eager float32 torch: grouped conv2d ("same"), blur(x^2) - mu^2."""
    C = image.shape[-1]
    i = torch.arange(window_size, dtype=torch.float64)
    g = torch.exp(-(i - (window_size - 1) / 2.0) ** 2 / (2.0 * sigma ** 2))
    g = (g / g.sum()).float().to(image.device)
    kernel = (g[:, None] * g[None, :]).expand(C, 1, window_size, window_size).contiguous()
    conv = lambda t: F.conv2d(t, kernel, padding=window_size // 2, groups=C)
    x, y = image.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)
    c1, c2 = k1 ** 2, k2 ** 2
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    return (((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))).mean()


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters   # us


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--batch", type=int, default=32)
    parser.add_argument("--size", type=int, default=1024)
    parser.add_argument("--iters", type=int, default=5)
    parser.add_argument("--repeats", type=int, default=5)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ssim_bench.py needs the MI355X: there is no fallback")
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand(B, S, S, 4, device=dev, generator=gen)
    image = (target + 0.05 * torch.randn(B, S, S, 4, device=dev, generator=gen)).clamp_(0, 1).requires_grad_(True)

    def step(loss_fn):
        image.grad = None
        value = loss_fn(image, target)
        value.backward()
        return value

    fused = lambda: step(losses.ssim)
    eager = lambda: step(eager_float32_ssim)
    value_fused = float(fused())
    grad_fused = image.grad.clone()
    value_eager = float(eager())
    grad_scale = float(image.grad.abs().max())
    grad_diff = float((image.grad - grad_fused).abs().max())
    del grad_fused
    for _ in range(2):   # warm-up
        fused()
        eager()
    torch.cuda.synchronize()
    pixels = B * S * S
    rows = []
    for _ in range(args.repeats):
        rows.append((timed(fused, args.iters), timed(eager, args.iters)))
        print(json.dumps({"fused_us": round(rows[-1][0], 1), "eager_us": round(rows[-1][1], 1)}), flush=True)
    fused_us, eager_us = statistics.median(r[0] for r in rows), statistics.median(r[1] for r in rows)
    print(json.dumps({
        "shape": [B, S, S, 4], "window": 11, "iters": args.iters, "repeats": args.repeats,
        "fused_forward_backward_us": round(fused_us, 1), "eager_forward_backward_us": round(eager_us, 1),
        "eager_over_fused": round(eager_us / fused_us, 2),
        "fused_spread_us": [round(min(r[0] for r in rows), 1), round(max(r[0] for r in rows), 1)],
        "eager_spread_us": [round(min(r[1] for r in rows), 1), round(max(r[1] for r in rows), 1)],
        "fused_algorithmic_bytes_per_pixel": BYTES_PER_PIXEL,
        "fused_fraction_of_8TBs": round(BYTES_PER_PIXEL * pixels / (fused_us * 1e-6) / PEAK, 3),
        "value_fused": value_fused, "value_eager": value_eager, "value_difference": abs(value_fused - value_eager),
        "gradient_max_difference_over_scale": grad_diff / grad_scale}), flush=True)


if __name__ == "__main__":
    main()
