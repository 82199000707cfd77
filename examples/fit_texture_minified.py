"""Recover a fine texture from small images: bilinear against mipmapped trilinear filtering.

Renders the K = 50 UV sphere with a known 512 x 512 texture from four cameras at 128 x 128 -- two to four texels per
pixel step at the centre of the disc, more towards its limb -- and recovers the texture from constant grey by Adam
through render_textured_filtered(), once with filter_mode="linear" and once with "linear-mipmap-linear".  A minified
bilinear lookup touches four texels per pixel, so most of the fine texture never receives a gradient and what does
is aliased; the mipmapped lookup spreads each pixel's gradient over its whole footprint.  Neither fit can recover
detail finer than a pixel, so the two are compared after box-filtering the recovered and the true texture to pyramid
level 2 (128 x 128).

    python examples/fit_texture_minified.py [--steps 100] [--size 128]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_mesh_renderer_amd import mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

TEXTURE_SIZE = 512
EYES = [[3.0, 0.6, 0.0], [-3.0, -0.6, 0.0], [0.0, 0.6, 3.0], [0.0, -0.6, -3.0]]


def true_texture(device):
    """[512, 512, 3] in [0.1, 0.9]: a smooth colour field (periodic in u) plus a 16 x 16 checker in blue."""
    c = (torch.arange(TEXTURE_SIZE, dtype=torch.float32, device=device) + 0.5) / TEXTURE_SIZE
    vv, uu = torch.meshgrid(c, c, indexing="ij")
    cell = torch.arange(TEXTURE_SIZE, device=device) // 32
    checker = ((cell[:, None] + cell[None, :]) % 2).float()
    return torch.stack([0.5 + 0.4 * torch.sin(2.0 * math.pi * uu), 0.5 + 0.4 * torch.cos(math.pi * vv),
                        0.2 + 0.6 * checker], -1)


def level2(tex):
    """The 4 x 4 box filter of a [H,W,C] texture: its pyramid level 2."""
    return torch.nn.functional.avg_pool2d(tex.permute(2, 0, 1).unsqueeze(0), 4)[0].permute(1, 2, 0)


def fit(filter_mode, steps=100, size=128, lr=0.05, device="cuda:0"):
    """Adam on the texture from grey -> the mean |error| of the recovered texture at pyramid level 2, before and
    after, and the first and last image loss."""
    device = torch.device(device)
    vertices, triangles, _ = shapes.sphere(1.0, 50)
    uvs, uv_triangles = shapes.sphere_uvs(50)
    B = len(EYES)
    vertices = vertices.unsqueeze(0).repeat(B, 1, 1).to(device)
    triangles, uvs, uv_triangles = triangles.to(device), uvs.to(device), uv_triangles.to(device)
    eyes = torch.tensor(EYES, device=device)
    center = torch.zeros(B, 3, device=device)
    up = torch.tensor([0.0, 1.0, 0.0], device=device)
    target_texture = true_texture(device)

    def image(tex):
        return mesh_renderer.render_textured_filtered(vertices, triangles, uvs, tex, eyes, center, up, size, size,
                                                      uv_triangles=uv_triangles, filter_mode=filter_mode)

    with torch.no_grad():
        # what a camera of this resolution sees of the true texture: the prefiltered image, for both fits
        target = mesh_renderer.render_textured_filtered(vertices, triangles, uvs, target_texture, eyes, center, up, size,
                                                        size, uv_triangles=uv_triangles,
                                                        filter_mode="linear-mipmap-linear")
    texture = torch.full((TEXTURE_SIZE, TEXTURE_SIZE, 3), 0.5, device=device, requires_grad=True)
    want = level2(target_texture)
    initial_error = float((level2(texture.detach()) - want).abs().mean())
    optimizer = torch.optim.Adam([texture], lr=lr)
    losses = []
    for _ in range(steps):
        optimizer.zero_grad()
        loss = torch.mean((image(texture) - target) ** 2)
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
    return {"filter_mode": filter_mode, "initial_loss": losses[0], "final_loss": losses[-1],
            "initial_level2_error": initial_error,
            "final_level2_error": float((level2(texture.detach()) - want).abs().mean())}


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--steps", type=int, default=100)
    parser.add_argument("--size", type=int, default=128)
    args = parser.parse_args()
    for mode in ("linear", "linear-mipmap-linear"):
        r = fit(mode, steps=args.steps, size=args.size)
        print("%-22s loss %.3g -> %.3g, level-2 texture error %.4f -> %.4f" % (
            mode, r["initial_loss"], r["final_loss"], r["initial_level2_error"], r["final_level2_error"]))


if __name__ == "__main__":
    main()
