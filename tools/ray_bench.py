"""Ray casting against a mesh, four legs alternating in one process:
  hip      mesh_renderer.points.cast_rays (the k_ray_* kernels of csrc/nearest.hip: 48-byte corner records in LDS read
           as broadcasts, one or two rays a lane in packed fp32, the watertight edge test with everything after the
           sign test behind a branch)
  torch    the package's own chunked torch expression of the same definition on the device
           (mesh_renderer.points._cast_rays_torch) -- what a float64 or host tensor takes
  winding  mesh_renderer.points.winding_number with the ray origins as the queries: the all-pairs sum on the same frame
  nearest  mesh_renderer.points.nearest_triangles with the ray origins as the queries
at (B 32, 20 000 rays x 5000 triangles) -- the benchmark sphere seen from a shell of sensors -- and (B 1, 100 000 x
200).  Device events after warm-up, the median of several groups, the garbage collector paused as bench.py pauses it.
Prints per shape the launch plan, the times, the (ray, triangle) pairs per second of the three HIP legs, the share of
rays that hit and whether the two spellings of cast_rays agree.

    python tools/ray_bench.py [--iters 10] [--torch-iters 1] [--groups 5] [--shapes 32x20000x5000,1x100000x200]

One JSON line per shape on standard output; the committed table is that output redirected:
    python tools/ray_bench.py > profiles/ray_bench.txt
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
    # sensors on a shell of radius 3 around the sphere, aimed at points of the ball of radius 1.3: most rays hit
    origins = 3.0 * torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g), dim=-1)
    aims = 1.3 * torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g), dim=-1) * torch.rand(B, N, 1, generator=g) ** (1 / 3)
    origins, directions = origins.to(dev), (aims - origins).to(dev)
    long_tri = tri.long()

    legs = {"hip_us": (lambda: points.cast_rays(origins, directions, v, tri), iters),
            "torch_us": (lambda: points._cast_rays_torch(origins, directions, v, long_tri, None, 0.0, float("inf")),
                         torch_iters),
            "winding_number_us": (lambda: points.winding_number(origins, v, tri), iters),
            "nearest_triangles_us": (lambda: points.nearest_triangles(origins, v, tri), iters)}
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
        a = points.cast_rays(origins, directions, v, tri)
        b = points._cast_rays_torch(origins, directions, v, long_tri, None, 0.0, float("inf"))
    result = {"B": B, "N": N, "V": v.shape[1], "T": T, "plan": _native.cast_rays_plan(B, N, T)}
    for name, values in samples.items():
        result[name] = round(statistics.median(values), 1)
    pairs = float(B) * N * T
    result["pairs"] = pairs
    for leg in ("hip", "winding_number", "nearest_triangles"):
        result[leg + "_pairs_per_s"] = round(pairs / (result[leg + "_us"] * 1e-6), 0)
    result["rate_over_winding_number"] = round(result["winding_number_us"] / result["hip_us"], 3)
    result["speedup_over_torch"] = round(result["torch_us"] / result["hip_us"], 2)
    same = a[1] == b[1]
    result["hit_share"] = float((a[1] >= 0).float().mean())
    result["faces_agree_share"] = float(same.float().mean())
    hit = same & (a[1] >= 0)
    result["max_t_difference"] = float((a[0] - b[0])[hit].abs().max()) if bool(hit.any()) else 0.0
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
