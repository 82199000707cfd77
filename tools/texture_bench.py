"""Texture sampling kernels at the bench shape: 5k sphere mapped with shapes.sphere_uvs, 1024^2, B = 32, one RGB
texture shared by the batch, at Wt = Ht in {256, 1024, 4096} (magnified, matched, minified).  The UV buffer and the
coverage mask come from the rasterizer and the interpolator once; then the sampler alone is timed with hip events.
Prints microseconds and the fraction of 8 TB/s over the per-pixel algorithmic bytes (texture traffic not counted),
and the fraction of the backward's 64 x 16 tiles whose footprint fits the LDS window of either mode:
  forward   read uv 8 + mask 4 B/px, write 3 channels 12 B/px                        (24 B/px)
  backward  read dout 12 + uv 8 + mask 4 B/px, write duv 8 B/px                       (32 B/px)
            (float atomics, and the deterministic mode: set_deterministic(True))

--filter linear-mipmap-linear (or both, in one session) times the mipmapped trilinear sampler on the same job: uv_da
from attribute_derivatives once, then mr_texture_mip_forward (pyramid build + sampling; it also writes uv_da's
16 B/px) and mr_texture_mip_backward (scatter into the gradient pyramid + fold).  Per-kernel times of k_mip_build,
k_tex_mip_forward, k_tex_mip_backward and k_mip_fold: run this tool under rocprofv3 --kernel-trace --stats.

    python tools/texture_bench.py [--batch 32] [--size 1024] [--textures 256,1024,4096] [--iters 20]
                                  [--filter linear|linear-mipmap-linear|both]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_mesh_renderer_amd import _native
from pytorch_mesh_renderer_amd.common import camera_utils, shapes, synthetic

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


def tile_paths(uv, mask, St, C=3):
    """The backward's 64 x 16 pixel tiles (csrc/texture.hip, wrap mode) -> (tiles that sample any texel, those whose
    unwrapped tap box x C fits the float LDS window (8192 cells), those that fit the fixed-point window (4096
    cells)).  The others take the wavefront-merged per-lane atomics."""
    f32 = torch.float32
    x = uv[..., 0] * torch.tensor(float(St), dtype=f32, device=uv.device) - torch.tensor(0.5, dtype=f32, device=uv.device)
    y = uv[..., 1] * torch.tensor(float(St), dtype=f32, device=uv.device) - torch.tensor(0.5, dtype=f32, device=uv.device)
    valid = (mask > 0.5) & (x.abs() < 2.0 ** 24) & (y.abs() < 2.0 ** 24)
    B, H, W = valid.shape
    ph, pw, big = -H % 16, -W % 64, 1 << 40

    def tiles(t, fill):
        t = torch.where(valid, t, torch.full_like(t, fill))
        return torch.nn.functional.pad(t, (0, pw, 0, ph), value=fill).view(B, (H + ph) // 16, 16, (W + pw) // 64, 64)
    x0, y0 = torch.floor(torch.where(valid, x, 0.0)).long(), torch.floor(torch.where(valid, y, 0.0)).long()
    bx0, by0 = tiles(x0, big).amin((2, 4)), tiles(y0, big).amin((2, 4))
    bx1, by1 = tiles(x0 + 1, -big).amax((2, 4)), tiles(y0 + 1, -big).amax((2, 4))
    used = bx0 <= bx1
    cells = (bx1 - bx0 + 1) * (by1 - by0 + 1) * C
    return int(used.sum()), int((used & (cells <= 8192)).sum()), int((used & (cells <= 4096)).sum())


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--batch", type=int, default=32)
    parser.add_argument("--size", type=int, default=1024)
    parser.add_argument("--textures", default="256,1024,4096")
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--filter", default="linear", choices=["linear", "linear-mipmap-linear", "both"])
    args = parser.parse_args()
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    job = synthetic.sphere_job(B, S, S)
    vertices, tris = job["vertices"].to(dev), job["triangles"].to(dev)
    uvs, uv_tris = shapes.sphere_uvs(50)
    uvs, uv_tris = uvs.to(dev), uv_tris.to(dev)
    with torch.no_grad():
        clip = camera_utils.transform_homogeneous(synthetic.clip_transforms(job["eyes"], S, S).to(dev), vertices)
        ids, bary, _ = _native.rasterize_forward(clip.contiguous(), tris, S, S)
        attrs = torch.cat([uvs, torch.ones(uvs.shape[0], 1, device=dev)], 1).unsqueeze(0).expand(B, -1, -1)
        px = _native.interpolate_forward(ids, bary, attrs.contiguous(), uv_tris, torch.zeros(3, device=dev))
        uv_da = None
        if args.filter != "linear":
            uv_da = _native.attribute_derivatives(ids, bary, clip.contiguous(), tris,
                                                  uvs.unsqueeze(0).expand(B, -1, -1).contiguous(), uv_tris).view(B, S, S, 4)
    uv, mask = px[..., 0:2].contiguous(), px[..., 2].contiguous()
    del ids, bary, px
    dout = torch.randn(B, S, S, 3, device=dev)
    pixels = B * S * S
    results = []
    filters = ["linear", "linear-mipmap-linear"] if args.filter == "both" else [args.filter]
    for St in [int(t) for t in args.textures.split(",")]:
        tex = torch.rand(St, St, 3, device=dev)
        for mode in filters:
            if mode == "linear":
                forward = lambda: _native.texture_forward(tex, uv, mask, "wrap")
                backward = lambda: _native.texture_backward(dout, tex, uv, mask, "wrap")
            else:
                pyramid = _native.texture_mip_forward(tex, uv, uv_da, mask, "wrap")[1]
                forward = lambda: _native.texture_mip_forward(tex, uv, uv_da, mask, "wrap")
                backward = lambda: _native.texture_mip_backward(dout, tex, pyramid, uv, uv_da, mask, "wrap")
            fwd_us = timed(forward, args.iters)
            bwd_us = timed(backward, args.iters)
            before = _native.set_deterministic(True)
            try:
                det_us = timed(backward, args.iters)
            finally:
                _native.set_deterministic(before)
            row = {"filter": mode, "shape": [B, S, S], "texture": [St, St, 3],
                   "covered_fraction": round(float((mask > 0.5).float().mean()), 3),
                   "forward_us": round(fwd_us, 1), "backward_us": round(bwd_us, 1),
                   "backward_deterministic_us": round(det_us, 1)}
            if mode == "linear":
                used, fit_float, fit_fixed = tile_paths(uv, mask, St)
                row.update({
                    "tiles_sampling": used, "tiles_in_float_window": round(fit_float / max(used, 1), 3),
                    "tiles_in_fixed_window": round(fit_fixed / max(used, 1), 3),
                    "forward_fraction_of_8TBs": round(24 * pixels / (fwd_us * 1e-6) / PEAK, 3),
                    "backward_fraction_of_8TBs": round(32 * pixels / (bwd_us * 1e-6) / PEAK, 3),
                    "backward_deterministic_fraction_of_8TBs": round(32 * pixels / (det_us * 1e-6) / PEAK, 3)})
            else:
                lod = 0.5 * torch.log2(torch.maximum((uv_da[..., 0] * St) ** 2 + (uv_da[..., 2] * St) ** 2,
                                                     (uv_da[..., 1] * St) ** 2 + (uv_da[..., 3] * St) ** 2))
                lod = lod[mask > 0.5].clamp(0, _native.texture_mip_levels(St, St) - 1)
                row.update({"levels": _native.texture_mip_levels(St, St), "median_lod": round(float(lod.median()), 2)})
            print(json.dumps(row), flush=True)
        del tex


if __name__ == "__main__":
    main()
