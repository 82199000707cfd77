"""Winding number of a mesh around a scan's points, three legs alternating in one process:
  hip      mesh_renderer.points.winding_number (the k_wn_* kernels of csrc/nearest.hip: 48-byte triangle records in LDS
           read as broadcasts, one or two queries a lane in packed fp32, a 64-bit fixed-point sum per query)
  torch    the package's own chunked torch expression of the same formula on the device
           (mesh_renderer.points._winding_number_torch) -- what a float64 or host tensor takes
  nearest  mesh_renderer.points.nearest_triangles on the same inputs: the distance search whose frame the sum shares
at (B 32, 20 000 points x 5000 triangles) -- the benchmark sphere against a scan -- and (B 1, 100 000 x 200).  Device
events after warm-up, the median of several groups, the garbage collector paused as bench.py pauses it.  Prints per
shape the launch plan, the times, the (point, triangle) pairs per second of both HIP legs and the largest difference
between the two spellings of the winding number.

    python tools/winding_bench.py [--iters 10] [--torch-iters 1] [--groups 5] [--shapes 32x20000x5000,1x100000x200]

One JSON line per shape on standard output; the committed table is that output redirected:
    python tools/winding_bench.py > profiles/winding_bench.txt
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
from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer import points


def mesh_of(B, T, generator):
    """A sphere of about T triangles (exactly T for 5000 and 200), jittered per image."""
    vertices, triangles, _ = shapes.sphere(1.0, max(2, int((T / 2.0) ** 0.5 + 1e-9)))   # 2 r^2 triangles
    v = vertices[None] + 0.01 * torch.randn(B, vertices.shape[0], 3, generator=generator)
    return v, triangles


def timed_group(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters   # us


def measure(B, N, T, iters, torch_iters, groups):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    v, tri = mesh_of(B, T, g)
    T = tri.shape[0]
    v, tri = v.to(dev), tri.to(dev)
    scan = (torch.randn(B, N, 3, generator=g) * 0.1 + torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g),
                                                                                    dim=-1)).to(dev)
    long_tri = tri.long()

    legs = {"hip_us": (lambda: points.winding_number(scan, v, tri), iters),
            "torch_us": (lambda: points._winding_number_torch(scan, v, long_tri, None), torch_iters),
            "nearest_triangles_us": (lambda: points.nearest_triangles(scan, v, tri), iters)}
    with torch.no_grad():
        for name, (fn, _) in legs.items():
            for _ in range(1 if name == "torch_us" else 3):
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name in legs}
        gc.collect()
        gc.disable()
        try:
            for _ in range(groups):
                for name, (fn, count) in legs.items():        # the legs alternate inside every group
                    samples[name].append(timed_group(fn, count))
        finally:
            gc.enable()
        a, b = points.winding_number(scan, v, tri), points._winding_number_torch(scan, v, long_tri, None)
    result = {"B": B, "N": N, "V": v.shape[1], "T": T, "plan": _native.winding_number_plan(B, N, T)}
    for name, values in samples.items():
        result[name] = round(statistics.median(values), 1)
    pairs = float(B) * N * T
    result["pairs"] = pairs
    result["hip_pairs_per_s"] = round(pairs / (result["hip_us"] * 1e-6), 0)
    result["nearest_triangles_pairs_per_s"] = round(pairs / (result["nearest_triangles_us"] * 1e-6), 0)
    result["speedup_over_torch"] = round(result["torch_us"] / result["hip_us"], 2)
    result["max_difference"] = float((a - b).abs().max())
    result["inside_share"] = float((a >= 0.5).float().mean())
    return result


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--iters", type=int, default=10)
    parser.add_argument("--torch-iters", type=int, default=1)
    parser.add_argument("--groups", type=int, default=5)
    parser.add_argument("--shapes", default="32x20000x5000,1x100000x200")
    args = parser.parse_args()
    for shape in args.shapes.split(","):
        B, N, T = (int(x) for x in shape.split("x"))
        print(json.dumps(measure(B, N, T, args.iters, args.torch_iters, args.groups)), flush=True)


if __name__ == "__main__":
    main()
