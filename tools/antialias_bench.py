"""Silhouette antialiasing kernels alone at the bench shape: 5k sphere, 1024^2, B = 32, RGBA of the
composed render (render(..., antialias=True)'s input).  Times the forward and the backward with hip events
and prints microseconds and the fraction of 8 TB/s over the algorithmic bytes:
  forward  read colour 16 + ids 4 + z 4 B/px, bary 12 B at id == 0 pixels, write 16 B/px
  backward read dout 16 + ids 4 + z 4 B/px, bary 12 B at id == 0 pixels, write dimage 16 B/px
(the colours at blended pairs and the clip / triangle reads are sparse and not counted).

    python tools/antialias_bench.py [--batch 32] [--size 1024] [--iters 20] [--deterministic]
"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import synthetic
render_module = importlib.import_module("pytorch_mesh_renderer_amd.mesh_renderer.render")  # (the package's `render` is the function)
from pytorch_mesh_renderer_amd.mesh_renderer.rasterize_triangles_ext import AttributeInterpolator

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
    parser.add_argument("--deterministic", action="store_true")
    args = parser.parse_args()
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    job = synthetic.sphere_job(B, S, S)
    clip, tris = job["clip"].to(dev), job["triangles"].to(dev)
    with torch.no_grad():
        ids, bary, z = _native.rasterize_forward(clip, tris, S, S)
        attrs = torch.cat([job["normals"], job["vertices"], job["diffuse"]], 2).to(dev)
        px = AttributeInterpolator.apply(ids, bary, attrs, tris, torch.full((9,), -1.0, device=dev))
        rgba = render_module._phong_rgba(torch.nn.functional.normalize(px[..., 0:3], p=2, dim=3),
                                         (px[..., 6:9] >= 0).any(dim=3).to(torch.float32), px[..., 3:6],
                                         job["light_positions"].to(dev), job["light_intensities"].to(dev),
                                         px[..., 6:9]).contiguous()
        del px, attrs
    opp = mesh_renderer.antialias_topology(tris, clip.shape[1])
    dout = torch.randn_like(rgba)
    _native.set_deterministic(args.deterministic)
    fwd_us = timed(lambda: _native.antialias_forward(rgba, ids, bary, z, clip, tris, opp), args.iters)
    bwd_us = timed(lambda: _native.antialias_backward(dout, rgba, ids, bary, z, clip, tris, opp), args.iters)
    out, mask = _native.antialias_forward(rgba, ids, bary, z, clip, tris, opp, want_pair_mask=True)
    pixels = B * S * S
    background = int((ids == 0).sum())
    nbytes = pixels * (16 + 4 + 4 + 16) + 12 * background
    blended = int(sum(((mask >> k) & 1).sum() for k in range(4)))
    result = {
        "shape": [B, S, S, 4], "deterministic": args.deterministic,
        "forward_us": round(fwd_us, 1), "backward_us": round(bwd_us, 1),
        "algorithmic_bytes": nbytes, "background_fraction": round(background / pixels, 4),
        "blended_pairs": blended,
        "forward_fraction_of_8TBs": round(nbytes / (fwd_us * 1e-6) / PEAK, 3),
        "backward_fraction_of_8TBs": round(nbytes / (bwd_us * 1e-6) / PEAK, 3),
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
