"""ICP between point clouds: what a round costs besides the search, and what launches cost the loop.  Per shape:
  search_us   mesh_renderer.points' nearest search of the moved cloud (_native.nearest_forward), one round's worth
  rest_us     the rest of a round: _native.align_apply and _native.align_solve through the idx plane (csrc/align.hip)
  loop_us     iterative_closest_point(check_every=0) at --rounds rounds, eager
  graph_us    the same loop captured once with torch.cuda.graph and replayed
  torch_us    the same rounds spelled in eager torch on the device: nearest_points, a gather, the weighted means, the
              covariance and torch.linalg.svd, with the convergence flag read back every round as the obvious loop does
              (null and the error's text where a step does not run on the device)
Device events after warm-up, the median of several groups, the legs alternating inside every group, the garbage
collector paused as bench.py pauses it.  x is y's first N points moved by 5 degrees, so every round does real work.

    python tools/icp_bench.py [--iters 3] [--groups 5] [--rounds 30] [--shapes 32x2000x20000,1x100000x100000]
"""
import argparse
import gc
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from pytorch_mesh_renderer_amd import _native
from pytorch_mesh_renderer_amd.mesh_renderer import points


def torch_icp(x, y, rounds):
    """The obvious eager loop: Kabsch with torch.linalg.svd on the device, rmse read back every round."""
    B = x.shape[0]
    R = torch.eye(3, device=x.device).repeat(B, 1, 1)
    T = x.new_zeros(B, 3)
    for _ in range(rounds):
        xt = x @ R + T[:, None]
        _, idx = points.nearest_points(xt, y)
        match = torch.gather(y, 1, idx.long()[..., None].expand(-1, -1, 3))
        xm, ym = x.mean(1), match.mean(1)
        C = (x - xm[:, None]).transpose(1, 2) @ (match - ym[:, None]) / x.shape[1]
        U, S, Vh = torch.linalg.svd(C.double())
        E = torch.ones(B, 3, dtype=torch.float64, device=x.device)
        E[:, 2] = torch.det(U @ Vh).sign()
        R = ((U * E[:, None, :]) @ Vh).float()
        T = ym - torch.einsum("bi,bij->bj", xm, R)
        # the read-back a convergence test needs; the value is not acted on, so that every leg runs every round
        float(((x @ R + T[:, None] - match) ** 2).sum(-1).mean().sqrt())
    return R, T


def timed_group(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters   # us


def measure(B, N, M, rounds, iters, groups):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    y = (torch.rand(B, M, 3, generator=g) * 2 - 1)
    t = math.radians(5.0)
    turn = torch.tensor([[math.cos(t), -math.sin(t), 0.0], [math.sin(t), math.cos(t), 0.0], [0.0, 0.0, 1.0]])
    x = (y[:, :N] @ turn + 0.02).to(dev)
    y = y.to(dev)
    run = lambda: points.iterative_closest_point(x, y, max_iterations=rounds, check_every=0)
    with torch.no_grad():
        first = run()
        _, idx, _ = _native.nearest_forward(x, y)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = run()

        def rest():
            R, T, s, _ = _native.align_solve(x, y, idx=idx, gather=True)
            _native.align_apply(x, R, T, s)

        legs = {"search_us": (lambda: _native.nearest_forward(x, y), iters), "rest_us": (rest, iters),
                "loop_us": (run, 1), "graph_us": (graph.replay, 1)}
        result = {"B": B, "N": N, "M": M, "rounds": rounds, "nearest_plan": _native.nearest_plan(B, N, M)}
        try:
            torch_icp(x, y, 2)
            legs["torch_us"] = (lambda: torch_icp(x, y, rounds), 1)
        except Exception as e:   # recorded, not hidden: whether torch.linalg.svd runs on the device is a finding
            result["torch_us"] = None
            result["torch_error"] = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])
        for fn, _ in legs.values():
            fn()
        torch.cuda.synchronize()
        samples = {name: [] for name in legs}
        gc.collect()
        gc.disable()
        try:
            for _ in range(groups):
                for name, (fn, n) in legs.items():
                    samples[name].append(timed_group(fn, n))
        finally:
            gc.enable()
        for name, values in samples.items():
            result[name] = round(statistics.median(values), 1)
        result["rest_over_search"] = round(result["rest_us"] / result["search_us"], 3)
        result["loop_per_round_us"] = round(result["loop_us"] / rounds, 1)
        result["graph_per_round_us"] = round(result["graph_us"] / rounds, 1)
        if result.get("torch_us"):
            result["torch_over_loop"] = round(result["torch_us"] / result["loop_us"], 1)
        graph.replay()
        torch.cuda.synchronize()
        result["graph_equals_eager"] = bool(torch.equal(captured.RTs.R, first.RTs.R) and torch.equal(captured.rmse, first.rmse))
        result["iterations"] = [int(first.iterations.min()), int(first.iterations.max())]
    return result


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--iters", type=int, default=3)
    parser.add_argument("--groups", type=int, default=5)
    parser.add_argument("--rounds", type=int, default=30)
    parser.add_argument("--shapes", default="32x2000x20000,1x100000x100000")
    args = parser.parse_args()
    for shape in args.shapes.split(","):
        B, N, M = (int(v) for v in shape.split("x"))
        print(json.dumps(measure(B, N, M, args.rounds, args.iters, args.groups)), flush=True)


if __name__ == "__main__":
    main()
