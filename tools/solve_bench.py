"""Time the Laplacian solve of mesh_renderer.preconditioning on the device: the HIP route eager, the same call as a
captured graph, and the same conjugate gradients as eager torch on the same device (forced).

    python tools/solve_bench.py [--out profiles/solve_bench.txt] [--quick]

Shapes: (32, 2502, 3), the benchmark sphere's vertices under the resident route, and a grid mesh beyond that route's
limit under the stepped one; lam = 19, tol = 1e-6, the right-hand side is (I + lam L) applied to the vertices, so
the solution is the mesh.  Every figure is the median of `--repeats` windows of device events around enough
back-to-back calls to fill `--window-ms`.  Reported per shape: the iterations the slowest system took, microseconds
a solve and microseconds an iteration (a solve / those iterations; on the stepped route with check_every = 0 the
launches of all max_iterations are paid, which the `per launched` column shows).
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_mesh_renderer_amd import _native
from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer import preconditioning

LAM, TOL = 19.0, 1e-6


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


def grid_mesh(rows, columns):
    """A rows x columns height field: -> (vertices [V,3], triangles [T,3] int32)."""
    i, j = torch.meshgrid(torch.arange(rows), torch.arange(columns), indexing="ij")
    x, y = j.float() / columns, i.float() / rows
    vertices = torch.stack([x, y, 0.1 * torch.sin(6.0 * x) * torch.cos(4.0 * y)], -1).reshape(-1, 3)
    a = (i[:-1, :-1] * columns + j[:-1, :-1]).reshape(-1)
    triangles = torch.cat([torch.stack([a, a + 1, a + columns], 1), torch.stack([a + 1, a + columns + 1, a + columns], 1)])
    return vertices, triangles.int()


def measure(name, B, vertices, triangles, max_iterations, window_ms, repeats, with_torch, emit):
    dev = torch.device("cuda:0")
    triangles = triangles.to(dev)
    V = vertices.shape[0]
    scale = torch.linspace(0.5, 1.5, B)[:, None, None]
    x = (vertices[None] * scale).to(dev).contiguous()
    topology = _native.mesh_topology(triangles, V)
    b = _native.laplacian_apply(x, topology, LAM)
    plan = _native.laplacian_solve_plan(V, 3)

    def hip():
        return _native.laplacian_solve(b, topology, LAM, TOL, max_iterations)

    got, iterations, residual = hip()
    most = max(int(iterations.max()), 1)
    error = float((got - x).norm() / x.norm())
    launched = most if plan["route"] == 1 else max_iterations
    eager = time_call(hip, window_ms, repeats)
    polled = time_call(lambda: _native.laplacian_solve(b, topology, LAM, TOL, max_iterations, check_every=16), window_ms,
                       repeats)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = hip()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured[0], got)
    replay = time_call(graph.replay, window_ms, repeats)
    emit("%s: B %d, V %d, route %d (%d x %d), %d iterations at most, residual %.1e, |x - mesh| / |mesh| %.1e" % (
        name, B, V, plan["route"], plan["workgroup_size"], plan["vertices_per_lane"], most, float(residual.max()), error))
    emit("  %-34s %10s %14s %14s" % ("", "us a solve", "us / iteration", "per launched"))
    for label, us, count in (("HIP, eager, check_every = 0", eager, launched), ("HIP, eager, check_every = 16", polled, most),
                             ("HIP, captured graph", replay, launched)):
        emit("  %-34s %10.1f %14.2f %14.2f" % (label, us, us / most, us / count))
    if with_torch:
        def loop():   # exactly the iterations the systems need: the loop's best case, nothing read back
            return preconditioning._solve_torch(b, topology, LAM, TOL, most, None, 0)

        theirs = loop()[0]
        assert float((theirs - got).norm() / got.norm()) < 1e-4
        us = time_call(loop, window_ms, 1, max_calls=8)
        emit("  %-34s %10.1f %14.2f %14.2f" % ("eager torch, the same CG, forced", us, us / most, us / most))
    emit("")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="short windows")
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=300)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("solve_bench.py measures on the GPU: there is nothing to time without one")
    if args.quick:
        args.window_ms, args.repeats = 10.0, 3
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit("# tools/solve_bench.py on %s, window %.0f ms x %d, lam %g, tol %g, max_iterations %d" % (
        torch.cuda.get_device_name(0), args.window_ms, args.repeats, LAM, TOL, args.max_iterations))
    sphere, sphere_triangles, _ = shapes.sphere(1.0, 50)
    measure("sphere", 32, sphere, sphere_triangles, args.max_iterations, args.window_ms, args.repeats,
            not args.no_torch, emit)
    vertices, triangles = grid_mesh(250, 400)
    measure("grid 250 x 400", 1, vertices, triangles, args.max_iterations, args.window_ms, args.repeats,
            not args.no_torch, emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
