"""Mesh regularisers, forward + backward of the three terms together, two spellings alternating in one process:
  torch   the fitting example's sparse Laplacian (torch.sparse.mm) and fancy-indexed edge loss
          (examples/fit_mesh_silhouettes.py, batched), plus a torch normal consistency over the same flaps
  hip     mesh_renderer.regularizers.mesh_regularizer (csrc/mesh_reg.hip: two forward launches, one backward)
at the benchmark mesh (sphere K = 50, V 2502, B = 32) and at sphere K = 200 (V 40 002, B = 16).  Device events
after warm-up, the median of several groups, the garbage collector paused as bench.py pauses it.  Also times the
two kernels' wrappers alone and prints their algorithmic bytes over time as a share of 8 TB/s:
  forward   read vertices 12 B, write unit directions 12 B per (image, vertex); the topology once
  backward  read vertices + unit directions 24 B, write dvertices 12 B per (image, vertex); the topology once
and the number of kernel launches of one step of each spelling (torch.profiler's kernel trace).

    python tools/regularizer_bench.py [--iters 20] [--groups 7] [--no-launch-count]
"""
import argparse
import gc
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from pytorch_mesh_renderer_amd import _native
from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer import regularizers

PEAK = 8.0e12
WEIGHTS = (0.1, 0.1, 0.05)


def _example():
    spec = importlib.util.spec_from_file_location("fit_mesh_silhouettes",
                                                  os.path.join(ROOT, "examples", "fit_mesh_silhouettes.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def torch_spelling(triangles, vertex_count, flaps):
    """-> f(vertices [B,V,3]) = the weighted sum per image, spelled as the example spells it."""
    example = _example()
    edges = example.compute_edges_list(triangles)
    laplacian = example.compute_laplacian(vertex_count, edges)
    flaps = flaps.long()

    def total(v):
        B, V, _ = v.shape
        delta = torch.sparse.mm(laplacian, v.permute(1, 0, 2).reshape(V, B * 3)).reshape(V, B, 3)
        lap = delta.norm(dim=2).sum(0) / V
        edge = (v[:, edges[:, 0]] - v[:, edges[:, 1]]).norm(dim=2, p=2).mean(1)
        a, b, c, d = v[:, flaps[:, 0]], v[:, flaps[:, 1]], v[:, flaps[:, 2]], v[:, flaps[:, 3]]
        n0 = torch.cross(b - a, c - a, dim=-1)
        n1 = torch.cross(d - a, b - a, dim=-1)
        nc = (1.0 - torch.nn.functional.cosine_similarity(n0, n1, dim=-1)).mean(1)
        return WEIGHTS[0] * lap + WEIGHTS[1] * edge + WEIGHTS[2] * nc
    return total


def timed_group(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters   # us


def launches(fn):
    """Kernel launches of one call of fn, from the profiler's kernel trace (None where it is not available)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as e:   # a measurement aid: the timings do not depend on it
        print("launch count unavailable: %s" % e, file=sys.stderr)
        return None


def measure(resolution, batch, iters, groups, count_launches):
    dev = torch.device("cuda:0")
    vertices, triangles, _ = shapes.sphere(1.0, resolution)
    V = vertices.shape[0]
    triangles = triangles.to(dev)
    g = torch.Generator().manual_seed(0)
    v = (vertices[None] + 0.01 * torch.randn(batch, V, 3, generator=g)).to(dev).requires_grad_(True)
    topology = regularizers.mesh_topology(triangles, V)
    spelled = torch_spelling(triangles, V, topology.flaps)

    def torch_step():
        v.grad = None
        spelled(v).sum().backward()

    def hip_step():
        v.grad = None
        regularizers.mesh_regularizer(v, triangles, *WEIGHTS).sum().backward()

    data = v.detach()
    dterms = torch.ones(batch, 3, device=dev)
    _, unit_dirs = _native.mesh_regularizer_forward(data, topology, 7)
    forward = lambda: _native.mesh_regularizer_forward(data, topology, 7)
    backward = lambda: _native.mesh_regularizer_backward(dterms, data, unit_dirs, topology, 7)
    legs = {"torch_step_us": torch_step, "hip_step_us": hip_step, "hip_forward_us": forward,
            "hip_backward_us": backward}
    for fn in legs.values():
        for _ in range(5):
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
    result = {"resolution": resolution, "batch": batch, "vertices": V, "edges": topology.edge_count,
              "flaps": topology.flap_count}
    for name, values in samples.items():
        result[name] = round(statistics.median(values), 1)
    E, F = topology.edge_count, topology.flap_count
    topo_fwd = 4 * (V + 1) + 8 * E + 16 * F
    topo_bwd = topo_fwd + 4 * (V + 1) + 16 * F
    result["forward_bytes"] = 24 * batch * V + topo_fwd
    result["backward_bytes"] = 36 * batch * V + topo_bwd
    result["forward_fraction_of_8TBs"] = round(result["forward_bytes"] / (result["hip_forward_us"] * 1e-6) / PEAK, 4)
    result["backward_fraction_of_8TBs"] = round(result["backward_bytes"] / (result["hip_backward_us"] * 1e-6) / PEAK, 4)
    if count_launches:
        result["torch_launches"] = launches(torch_step)
        result["hip_launches"] = launches(hip_step)
        result["hip_kernel_launches"] = launches(lambda: (forward(), backward()))
    return result


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--groups", type=int, default=7)
    parser.add_argument("--no-launch-count", action="store_true")
    args = parser.parse_args()
    for resolution, batch in ((50, 32), (200, 16)):
        print(json.dumps(measure(resolution, batch, args.iters, args.groups, not args.no_launch_count)))


if __name__ == "__main__":
    main()
