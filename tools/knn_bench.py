"""K nearest neighbours between point clouds, forward only, three spellings alternating in one process:
  torch    the N x M distance tensor in the difference form, chunked over the queries so that a chunk stays near
           64 MB, torch.topk(..., largest=False) over the targets
  knn      mesh_renderer.points.knn_points (csrc/nearest.hip: a sorted list of K keys per query in registers)
  nearest  mesh_renderer.points.nearest_points at the same shape: the K = 1 search without a list
at (B 8, 10k x 10k), at (B 32, 2502 x 20k) and, HIP only since the torch spelling is not worth waiting for, at
(B 1, 100k x 100k), each at K in {1, 4, 16, 32}.  Device events after warm-up, the median of several groups, the
garbage collector paused as bench.py pauses it.  Prints per (shape, K) the launch plan, the times, the (query,
target) pairs per second of knn_points and its time as a multiple of nearest_points' in the same run: that ratio is
the measured cost of the list, and the only evidence there is of how often a wavefront walks the insertion chain.

    python tools/knn_bench.py [--iters 5] [--groups 5] [--shapes 8x10000x10000,...] [--ks 1,4,16,32]
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

TORCH_LIMIT_PAIRS = 4e9          # the torch spelling is skipped beyond this many (query, target) pairs
CHUNK_BYTES = 64 << 20


def torch_knn(x, y, K):
    """(sqdist [B,N,K], idx [B,N,K]) by torch.topk over the chunked distance tensor."""
    B, N, _ = x.shape
    rows = max(1, CHUNK_BYTES // (B * y.shape[1] * 3 * 4))
    values, indices = [], []
    for start in range(0, N, rows):
        diff = x[:, start:start + rows, None, :] - y[:, None, :, :]
        found = torch.topk((diff * diff).sum(-1), K, dim=2, largest=False)
        values.append(found.values)
        indices.append(found.indices)
    return torch.cat(values, dim=1), torch.cat(indices, dim=1)


def timed_group(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters   # us


def measure(B, N, M, K, iters, groups):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)
    y = (torch.rand(B, M, 3, generator=g) * 2 - 1).to(dev)
    with_torch = float(B) * N * M <= TORCH_LIMIT_PAIRS
    legs = {"knn_us": (lambda: points.knn_points(x, y, K), iters),
            "nearest_us": (lambda: points.nearest_points(x, y), iters)}
    if with_torch:
        legs["torch_topk_us"] = (lambda: torch_knn(x, y, K), 1)
    with torch.no_grad():
        for fn, _ in legs.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name in legs}
        gc.collect()
        gc.disable()
        try:
            for _ in range(groups):
                for name, (fn, n) in legs.items():        # the spellings alternate inside every group
                    samples[name].append(timed_group(fn, n))
        finally:
            gc.enable()
        result = {"B": B, "N": N, "M": M, "K": K, "plan": _native.knn_plan(B, N, M, K),
                  "nearest_plan": _native.nearest_plan(B, N, M)}
        for name, values in samples.items():
            result[name] = round(statistics.median(values), 1)
        pairs = float(B) * N * M
        result["knn_pairs_per_s"] = round(pairs / (result["knn_us"] * 1e-6), 0)
        result["nearest_pairs_per_s"] = round(pairs / (result["nearest_us"] * 1e-6), 0)
        result["knn_over_nearest"] = round(result["knn_us"] / result["nearest_us"], 2)
        if with_torch:
            result["torch_over_knn"] = round(result["torch_topk_us"] / result["knn_us"], 1)
            a, b = points.knn_points(x, y, K)[0], torch_knn(x, y, K)[0]
            result["max_rel_difference"] = float(((a - b).abs() / b.clamp(min=1e-30)).max())
    return result


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--iters", type=int, default=5)
    parser.add_argument("--groups", type=int, default=5)
    parser.add_argument("--shapes", default="8x10000x10000,32x2502x20000,1x100000x100000")
    parser.add_argument("--ks", default="1,4,16,32")
    args = parser.parse_args()
    for shape in args.shapes.split(","):
        B, N, M = (int(v) for v in shape.split("x"))
        for K in (int(v) for v in args.ks.split(",")):
            print(json.dumps(measure(B, N, M, K, args.iters, args.groups)), flush=True)


if __name__ == "__main__":
    main()
