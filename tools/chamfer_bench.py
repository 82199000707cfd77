"""Chamfer distance, forward and forward + backward, two spellings alternating in one process:
  torch   the N x M distance tensor in the difference form, chunked over the queries so that a chunk stays near
          64 MB, min over the targets, the means, autograd through it (each chunk's graph keeps its tensor)
  hip     mesh_renderer.points.chamfer_distance (csrc/nearest.hip: brute-force nearest neighbours in registers and
          LDS, a fixed-order mean, a gathered backward over an inverted index)
at (B 8, 10k x 10k), at (B 32, 2502 x 20k) -- the benchmark sphere's vertices against a scan -- and, hip only since
torch cannot hold it, at (B 1, 100k x 100k).  Device events after warm-up, the median of several groups, the garbage
collector paused as bench.py pauses it.  Prints per shape the launch plan of both directions, the times, the
(query, target) pairs per second of the hip forward (both directions: 2 B N M pairs) and that rate as a share of the
FP32 vector peak at 8 flop-slots (vector instructions) per pair.

    python tools/chamfer_bench.py [--iters 10] [--groups 5] [--shapes 8x10000x10000,32x2502x20000,1x100000x100000]
"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from pytorch_mesh_renderer_amd import _native
from pytorch_mesh_renderer_amd.mesh_renderer import points

PEAK_FP32_VECTOR = 157.3e12      # MI355X spec sheet, FP32 vector: counts a fused multiply-add as two
INSTRUCTIONS_PER_PAIR = 8        # 3 subtractions, a product, 2 fused multiply-adds, a compare, (two selects as one)
TORCH_LIMIT_BYTES = 64 << 30     # the torch spelling's autograd graph holds every chunk: skip shapes beyond this
CHUNK_BYTES = 64 << 20


def torch_directed(x, y):
    """mean_i min_j |x_i - y_j|^2 per image, chunked over the queries."""
    B, N, _ = x.shape
    rows = max(1, CHUNK_BYTES // (B * y.shape[1] * 3 * 4))
    best = []
    for start in range(0, N, rows):
        diff = x[:, start:start + rows, None, :] - y[:, None, :, :]
        best.append((diff * diff).sum(-1).min(dim=2).values)
    return torch.cat(best, dim=1).mean(1)


def torch_chamfer(x, y):
    return torch_directed(x, y) + torch_directed(y, x)


def timed_group(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters   # us


def measure(B, N, M, iters, groups):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev).requires_grad_(True)
    y = (torch.rand(B, M, 3, generator=g) * 2 - 1).to(dev)
    with_torch = 2 * B * N * M * 3 * 4 <= TORCH_LIMIT_BYTES

    def hip_forward():
        with torch.no_grad():
            points.chamfer_distance(x, y)

    def hip_step():
        x.grad = None
        points.chamfer_distance(x, y).sum().backward()

    def torch_forward():
        with torch.no_grad():
            torch_chamfer(x, y)

    def torch_step():
        x.grad = None
        torch_chamfer(x, y).sum().backward()

    legs = {"hip_forward_us": hip_forward, "hip_step_us": hip_step}
    if with_torch:
        legs.update({"torch_forward_us": torch_forward, "torch_step_us": torch_step})
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in legs}
    gc.collect()
    gc.disable()
    try:
        for _ in range(groups):
            for name, fn in legs.items():        # the spellings alternate inside every group
                samples[name].append(timed_group(fn, iters))
    finally:
        gc.enable()
    result = {"B": B, "N": N, "M": M, "plan_xy": _native.nearest_plan(B, N, M), "plan_yx": _native.nearest_plan(B, M, N)}
    for name, values in samples.items():
        result[name] = round(statistics.median(values), 1)
    pairs = 2.0 * B * N * M
    result["pairs"] = pairs
    result["hip_forward_pairs_per_s"] = round(pairs / (result["hip_forward_us"] * 1e-6), 0)
    result["hip_forward_share_of_fp32_vector_peak"] = round(
        result["hip_forward_pairs_per_s"] * INSTRUCTIONS_PER_PAIR * 2 / PEAK_FP32_VECTOR, 4)
    if with_torch:
        result["forward_speedup"] = round(result["torch_forward_us"] / result["hip_forward_us"], 2)
        result["step_speedup"] = round(result["torch_step_us"] / result["hip_step_us"], 2)
        with torch.no_grad():
            a, b = points.chamfer_distance(x, y), torch_chamfer(x, y)
        result["max_rel_difference"] = float(((a - b).abs() / b).max())
    return result


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--iters", type=int, default=10)
    parser.add_argument("--groups", type=int, default=5)
    parser.add_argument("--shapes", default="8x10000x10000,32x2502x20000,1x100000x100000")
    args = parser.parse_args()
    for shape in args.shapes.split(","):
        B, N, M = (int(v) for v in shape.split("x"))
        print(json.dumps(measure(B, N, M, args.iters, args.groups)), flush=True)


if __name__ == "__main__":
    main()
