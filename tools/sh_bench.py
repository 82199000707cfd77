"""Spherical-harmonics shading kernels at the bench shape: 5k sphere, 1024^2, B = 32, on the packed [B,H,W,6]
[normals, diffuse] buffer rasterize() gives render_sh().  Times with hip events and prints microseconds and the
fraction of 8 TB/s over the algorithmic bytes:
  forward   read normals + diffuse 24 B/px, write RGBA 16 B/px                         (40 B/px)
  backward  read drgba 16 + normals + diffuse 24 B/px, write dnormals + ddiffuse 24 B/px  (64 B/px)
  step      render_sh + L1 loss + backward (rasterizer and interpolation included; no byte model)

    python tools/sh_bench.py [--batch 32] [--size 1024] [--iters 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import synthetic

PEAK = 8.0e12


def timed(fn, iters):
    for _ in range(3):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
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
    parser.add_argument("--iters", type=int, default=20)
    args = parser.parse_args()
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    job = synthetic.sphere_job(B, S, S)
    vertices, tris = job["vertices"].to(dev), job["triangles"].to(dev)
    normals, diffuse = job["normals"].to(dev), (job["diffuse"] * 0.8).to(dev)
    sh = (torch.randn(B, 9, 3, generator=torch.Generator().manual_seed(0)) * 0.3).to(dev)
    sh[:, 0] += 1.0
    with torch.no_grad():
        packed = mesh_renderer.rasterize(vertices, torch.cat([normals, diffuse], 2),
                                         tris, synthetic.clip_transforms(job["eyes"], S, S).to(dev), S, S,
                                         torch.full((6,), -1.0, device=dev)).contiguous()
    n_in, d_in = packed[..., 0:3], packed[..., 3:6]
    drgba = torch.randn(B, S, S, 4, device=dev)
    fwd_us = timed(lambda: _native.sh_shade_forward(n_in, d_in, None, sh), args.iters)
    bwd_us = timed(lambda: _native.sh_shade_backward(drgba, n_in, d_in, None, sh, packed_grad=True), args.iters)
    del packed, n_in, d_in, drgba

    v = vertices.clone().requires_grad_(True)
    s = sh.clone().requires_grad_(True)
    eyes = job["eyes"].to(dev)
    center, up = torch.zeros(B, 3, device=dev), torch.tensor([[0.0, 1.0, 0.0]], device=dev).repeat(B, 1)
    with torch.no_grad():
        target = mesh_renderer.render_sh(vertices, tris, normals, diffuse, sh * 0.9, eyes, center, up, S, S)

    def step():
        v.grad = s.grad = None
        image = mesh_renderer.render_sh(v, tris, normals, diffuse, s, eyes, center, up, S, S)
        torch.mean(torch.abs(image - target)).backward()

    step_us = timed(step, max(3, args.iters // 4))
    pixels = B * S * S
    result = {
        "shape": [B, S, S], "triangles": int(tris.shape[0]),
        "forward_us": round(fwd_us, 1), "backward_us": round(bwd_us, 1), "step_us": round(step_us, 1),
        "forward_bytes": 40 * pixels, "backward_bytes": 64 * pixels,
        "forward_fraction_of_8TBs": round(40 * pixels / (fwd_us * 1e-6) / PEAK, 3),
        "backward_fraction_of_8TBs": round(64 * pixels / (bwd_us * 1e-6) / PEAK, 3),
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
