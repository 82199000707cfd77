"""Recover an RGB texture from images of a textured sphere.

Renders the K = 50 sphere, mapped with shapes.sphere_uvs (equirectangular, seam-free per-corner UVs), from six
axis-aligned cameras with a known 64 x 32 texture (a smooth colour field plus a checker), unlit.  Then recovers the
texture from constant grey by Adam through render_textured().  Every texel the views see receives a gradient
through the bilinear sampler's texture scatter.

    python examples/fit_texture.py --out /tmp/frames [--steps 300] [--size 128]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from PIL import Image

from pytorch_mesh_renderer_amd import mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

TEXTURE_W, TEXTURE_H = 64, 32
# six cameras on the axes; the two on the y axis look down / up with z as their up vector
EYES = [[3.0, 0.0, 0.0], [-3.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, -3.0, 0.0], [0.0, 0.0, 3.0], [0.0, 0.0, -3.0]]
UPS = [[0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0]]


def true_texture(device):
    """[32, 64, 3] in [0.1, 0.9]: a smooth colour field (periodic in u) plus an 8 x 4 checker in blue."""
    v = (torch.arange(TEXTURE_H, dtype=torch.float32, device=device) + 0.5) / TEXTURE_H
    u = (torch.arange(TEXTURE_W, dtype=torch.float32, device=device) + 0.5) / TEXTURE_W
    vv, uu = torch.meshgrid(v, u, indexing="ij")
    checker = ((torch.arange(TEXTURE_H, device=device)[:, None] // 8
                + torch.arange(TEXTURE_W, device=device)[None, :] // 8) % 2).float()
    r = 0.5 + 0.4 * torch.sin(2.0 * math.pi * uu)
    g = 0.5 + 0.4 * torch.cos(math.pi * vv)
    b = 0.2 + 0.6 * checker
    return torch.stack([r, g, b], -1)


def fit(steps=300, size=128, lr=0.05, device="cuda:0", out=None):
    """Adam on the texture from grey; returns the first and last loss and the mean texel error, before and after,
    over the texels the views see (a total bilinear weight of at least one pixel)."""
    device = torch.device(device)
    vertices, triangles, _ = shapes.sphere(1.0, 50)
    uvs, uv_triangles = shapes.sphere_uvs(50)
    B = len(EYES)
    vertices = vertices.unsqueeze(0).repeat(B, 1, 1).to(device)
    triangles, uvs, uv_triangles = triangles.to(device), uvs.to(device), uv_triangles.to(device)
    eyes = torch.tensor(EYES, device=device)
    ups = torch.tensor(UPS, device=device)
    center = torch.zeros(B, 3, device=device)
    target_texture = true_texture(device)

    def image(tex):
        return mesh_renderer.render_textured(vertices, triangles, uvs, tex, eyes, center, ups, size, size,
                                             uv_triangles=uv_triangles)

    with torch.no_grad():
        target = image(target_texture)
    # the texels the views see: d(sum of every image's rgb) / d texel is the texel's total bilinear weight
    probe = torch.zeros_like(target_texture, requires_grad=True)
    image(probe)[..., :3].sum().backward()
    seen = probe.grad[..., 0] >= 1.0

    texture = torch.full((TEXTURE_H, TEXTURE_W, 3), 0.5, device=device, requires_grad=True)
    initial_error = float((texture.detach() - target_texture).abs().mean(-1)[seen].mean())
    optimizer = torch.optim.Adam([texture], lr=lr)
    schedule = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, steps)
    losses = []
    for step in range(steps):
        optimizer.zero_grad()
        loss = torch.mean((image(texture) - target) ** 2)
        loss.backward()
        optimizer.step()
        schedule.step()
        losses.append(float(loss.detach()))
        if out is not None and step % 20 == 0:
            save(image(texture.detach()), os.path.join(out, "frame_%03d.png" % step))
    with torch.no_grad():
        final = float(torch.mean((image(texture) - target) ** 2))
    if out is not None:
        save(target, os.path.join(out, "target.png"))
        save(image(texture.detach()), os.path.join(out, "fitted.png"))
        save_texture(texture.detach(), os.path.join(out, "texture_fitted.png"))
        save_texture(target_texture, os.path.join(out, "texture_target.png"))
    return {"initial_loss": losses[0], "final_loss": final, "initial_texel_error": initial_error,
            "final_texel_error": float((texture.detach() - target_texture).abs().mean(-1)[seen].mean()),
            "seen_texels": int(seen.sum())}


def save(images, path):
    """The batch side by side as one 8-bit RGB frame."""
    rgb = torch.cat(list(images[..., :3].detach().clamp(0, 1)), dim=1)
    Image.fromarray((rgb * 255).round().to(torch.uint8).cpu().numpy()).save(path)


def save_texture(tex, path):
    """Row 0 of a texture is v = 0 (the bottom): flipped to be stored top row first."""
    rgb = torch.flip(tex.clamp(0, 1), dims=[0])
    Image.fromarray((rgb * 255).round().to(torch.uint8).cpu().numpy()).save(path)


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--out", default=None)
    parser.add_argument("--steps", type=int, default=300)
    parser.add_argument("--size", type=int, default=128)
    args = parser.parse_args()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    result = fit(steps=args.steps, size=args.size, out=args.out)
    print("loss %.3g -> %.3g, mean texel error %.3g -> %.3g over %d seen texels" % (
        result["initial_loss"], result["final_loss"], result["initial_texel_error"], result["final_texel_error"],
        result["seen_texels"]))


if __name__ == "__main__":
    main()
