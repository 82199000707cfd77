"""Mesh-to-point distance, forward and forward + backward to the vertices, two spellings alternating in one process:
  torch   the package's own chunked torch expression (mesh_renderer.points._triangle_nearest_points_torch: the four
          candidates of every (point, triangle) pair of a chunk of triangles kept near 64 MB, the minimum over the
          points, then the differentiable distance to the chosen point) -- what a float64 or host tensor takes
  hip     mesh_renderer.points.mesh_point_distance (the k_tp_* kernels of csrc/nearest.hip: one triangle's record in a
          lane's registers, the points in LDS read as broadcasts, two a step in packed fp32, a fixed-order mean, a
          gathered backward over inverted indices)
at (B 8, 10k points x 5000 triangles), at (B 32, 20k x 5000) -- the benchmark sphere against a scan -- and at
(B 1, 100k x 200), a small mesh against a large cloud, where the cloud is split to fill the chip.  Device events
after warm-up, the median of several groups, the garbage collector paused as bench.py pauses it.  Prints per shape the
launch plan, the times and the (point, triangle) pairs per second of the hip forward; tools/point_mesh_bench.py
prints the same figure for the other direction.

    python tools/mesh_point_bench.py [--iters 10] [--torch-iters 1] [--groups 5]
                                     [--shapes 8x10000x5000,32x20000x5000,1x100000x200]

One JSON line per shape on standard output; the committed table is that output redirected:
    python tools/mesh_point_bench.py > profiles/mesh_point_bench.txt
"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from point_mesh_bench import mesh_of, timed_group
from pytorch_mesh_renderer_amd import _native
from pytorch_mesh_renderer_amd.mesh_renderer import points

TORCH_LIMIT_PAIRS = 4e9          # the torch spelling moves about 2 KB per pair: beyond this it is not run


def measure(B, N, T, iters, torch_iters, groups):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    v, tri = mesh_of(B, T, g)
    T = tri.shape[0]
    v, tri = v.to(dev).requires_grad_(True), tri.to(dev)
    scan = (torch.randn(B, N, 3, generator=g) * 0.1 + torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g),
                                                                                    dim=-1)).to(dev)
    with_torch = float(B) * N * T <= TORCH_LIMIT_PAIRS

    def torch_mean():
        sqdist, _, _, usable = points._triangle_nearest_points_torch(scan, v, tri, None)
        return sqdist.sum(1) / usable.clamp(min=1).to(sqdist.dtype)

    def hip_forward():
        with torch.no_grad():
            points.mesh_point_distance(scan, v, tri)

    def hip_step():
        v.grad = None
        points.mesh_point_distance(scan, v, tri).sum().backward()

    def torch_forward():
        with torch.no_grad():
            torch_mean()

    def torch_step():
        v.grad = None
        torch_mean().sum().backward()

    legs = {"hip_forward_us": (hip_forward, iters), "hip_step_us": (hip_step, iters)}
    if with_torch:
        legs.update({"torch_forward_us": (torch_forward, torch_iters), "torch_step_us": (torch_step, torch_iters)})
    for name, (fn, _) in legs.items():
        for _ in range(3 if name.startswith("hip") else 1):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in legs}
    gc.collect()
    gc.disable()
    try:
        for _ in range(groups):
            for name, (fn, count) in legs.items():        # the spellings alternate inside every group
                samples[name].append(timed_group(fn, count))
    finally:
        gc.enable()
    result = {"B": B, "N": N, "V": v.shape[1], "T": T, "plan": _native.nearest_point_of_triangle_plan(B, N, T)}
    for name, values in samples.items():
        result[name] = round(statistics.median(values), 1)
    pairs = float(B) * N * T
    result["pairs"] = pairs
    result["hip_forward_pairs_per_s"] = round(pairs / (result["hip_forward_us"] * 1e-6), 0)
    if with_torch:
        result["forward_speedup"] = round(result["torch_forward_us"] / result["hip_forward_us"], 2)
        result["step_speedup"] = round(result["torch_step_us"] / result["hip_step_us"], 2)
        with torch.no_grad():
            a, b = points.mesh_point_distance(scan, v, tri), torch_mean()
        result["max_rel_difference"] = float(((a - b).abs() / b).max())
    return result


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--iters", type=int, default=10)
    parser.add_argument("--torch-iters", type=int, default=1)
    parser.add_argument("--groups", type=int, default=5)
    parser.add_argument("--shapes", default="8x10000x5000,32x20000x5000,1x100000x200")
    args = parser.parse_args()
    for shape in args.shapes.split(","):
        B, N, T = (int(x) for x in shape.split("x"))
        print(json.dumps(measure(B, N, T, args.iters, args.torch_iters, args.groups)), flush=True)


if __name__ == "__main__":
    main()
