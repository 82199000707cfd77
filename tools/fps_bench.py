"""Time farthest-point sampling on the device: both routes of mr_farthest_forward forced, the launch shapes of the
one-workgroup route, and the torch loop of K steps on the same device and shapes.

    python tools/fps_bench.py [--out profiles/farthest_bench.txt] [--quick]

Every figure is the median of `--repeats` windows of device events around enough back-to-back calls to fill
`--window-ms`; every (route, shape) is warmed first.  Two tables:

  routes   per (B, N, K): route 1 with the plan's shape (N <= 24576), route 2, the torch loop; microseconds a call and
           a step, and which route the plan takes
  shapes   per N (B = 1, K = 256): route 1 under every (workgroup size, points per lane) that holds N

The plan's constants in csrc/farthest.hip (the table of shapes, the crossover) are set from these tables.  Before a
figure is taken every forced result is compared with the plan's: faster and different is not faster.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_mesh_renderer_amd import _native
from pytorch_mesh_renderer_amd.mesh_renderer import points as point_losses

RESIDENT_CAPACITY = 24576
SIZES, PER_LANE = (64, 256, 1024), (4, 8, 16, 20, 24)


def time_call(call, window_ms, repeats, max_calls=4096):
    """-> median microseconds of one call()."""
    call()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    call()
    stop.record()
    torch.cuda.synchronize()
    once = max(start.elapsed_time(stop), 1e-3)
    calls = int(min(max_calls, max(1, window_ms / once)))
    windows = []
    for _ in range(repeats):
        start.record()
        for _ in range(calls):
            call()
        stop.record()
        torch.cuda.synchronize()
        windows.append(1e3 * start.elapsed_time(stop) / calls)
    return statistics.median(windows)


def cloud(B, N, dev):
    generator = torch.Generator().manual_seed(1000 + N)
    return (2 * torch.rand(B, N, 3, generator=generator) - 1).to(dev)


def routes_table(grid, window_ms, repeats, with_torch, emit):
    emit("routes: microseconds a call (a step)")
    emit("%6s %9s %5s | %22s | %22s | %22s | %s" % ("B", "N", "K", "route 1 (plan's shape)", "route 2 (slices)",
                                                      "torch loop", "plan"))
    dev = torch.device("cuda:0")
    for B, N, K in grid:
        c = cloud(B, N, dev)
        plan = _native.farthest_plan(B, N, K)
        want = _native.farthest_forward(c, K)
        cells = []
        for route in (1, 2):
            if route == 1 and N > RESIDENT_CAPACITY:
                cells.append("%22s" % "-")
                continue
            got = _native.farthest_forward(c, K, route=route)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (B, N, K, route)
            us = time_call(lambda: _native.farthest_forward(c, K, route=route), window_ms, repeats)
            cells.append("%12.1f (%7.2f)" % (us, us / K))
        if with_torch:
            us = time_call(lambda: point_losses._farthest_torch(c, K, None, None), window_ms, 1, max_calls=4)
            cells.append("%12.1f (%7.2f)" % (us, us / K))
        else:
            cells.append("%22s" % "not measured")
        shape = ("%d x %d" % (plan["workgroup_size"], plan["points_per_lane"]) if plan["route"] == 1
                 else "%d slices" % plan["slices"])
        emit("%6d %9d %5d | %s | %s | %s | route %d, %s" % (B, N, K, cells[0], cells[1], cells[2], plan["route"], shape))


def shapes_table(sizes, window_ms, repeats, emit, K=256):
    emit("")
    emit("shapes: route 1, B = 1, K = %d, microseconds a step under (workgroup size x points per lane)" % K)
    emit("%9s | %s" % ("N", " ".join("%9s" % ("%dx%d" % (w, p)) for w in SIZES for p in PER_LANE)))
    dev = torch.device("cuda:0")
    try:
        for N in sizes:
            c = cloud(1, N, dev)
            steps = min(K, N)
            _native.debug_set_farthest_shape(0, 0)
            want = _native.farthest_forward(c, steps, route=2)
            cells = []
            for w in SIZES:
                for p in PER_LANE:
                    if w * p < N:
                        cells.append("%9s" % "-")
                        continue
                    _native.debug_set_farthest_shape(w, p)
                    got = _native.farthest_forward(c, steps, route=1)
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (N, w, p)
                    us = time_call(lambda: _native.farthest_forward(c, steps, route=1), window_ms, repeats)
                    cells.append("%9.3f" % (us / steps))
            emit("%9d | %s" % (N, " ".join(cells)))
    finally:
        _native.debug_set_farthest_shape(0, 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a small grid, short windows")
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fps_bench.py measures on the GPU: there is nothing to time without one")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit("# tools/fps_bench.py on %s, window %.0f ms x %d" % (torch.cuda.get_device_name(0), args.window_ms,
                                                             args.repeats))
    if args.quick:
        grid = [(1, 1024, 64), (1, 16384, 64), (1, 100000, 64)]
        sizes = [256, 4096]
    else:
        grid = [(B, N, K) for B in (1, 8)
                for N in (256, 1024, 4096, 8192, 16384, 24576, 40000, 100000, 1000000) for K in (64, 512)]
        sizes = [64, 256, 512, 1024, 2048, 4096, 6144, 8192, 16384, 20480, 24576]
    shapes_table(sizes, args.window_ms, args.repeats, emit)
    emit("")
    routes_table(grid, args.window_ms, args.repeats, not args.no_torch, emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
