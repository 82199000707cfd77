"""Recover a cube's horizontal offset from a target silhouette with the HARD rasterizer.

Without antialiasing the alpha of render() is binary and a silhouette loss has no gradient to the vertices;
render(..., antialias=True) blends the outline pixels by where the outline crosses them, so the same loss
pulls the mesh into place.

    python examples/fit_silhouette_antialiased.py --out /tmp/frames [--steps 150]
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

FOV_Y = 40.0


def fit(steps=150, width=128, height=96, true_offset=0.23, device="cuda:0", out=None):
    """Gradient descent on the offset [dx] of a cube from a target alpha; returns the final offset and its
    error in pixels (one pixel = the frame's width at the cube's depth / width)."""
    device = torch.device(device)
    cube_v, triangles, cube_n = shapes.cube(2.0)
    triangles = torch.flip(triangles, [1]).contiguous().to(device)   # CCW -> CW, as the examples do
    cube_v, cube_n = cube_v.to(device), cube_n.unsqueeze(0).to(device)
    distance = 7.0
    eye = torch.tensor([[0.0, 0.0, distance]], device=device)
    center, up = torch.zeros(1, 3, device=device), torch.tensor([[0.0, 1.0, 0.0]], device=device)
    light_positions = eye.unsqueeze(1)
    light_intensities = torch.ones(1, 1, 3, device=device)
    diffuse = torch.ones(1, 8, 3, device=device)
    rotation = torch.tensor([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]], device=device)
    base = cube_v @ rotation.T

    def alpha(offset):
        vertices = (base + torch.cat([offset, torch.zeros(2, device=device)])).unsqueeze(0)
        image = mesh_renderer.render(vertices, triangles, cube_n, diffuse, eye, center, up, light_positions,
                                     light_intensities, width, height, antialias=True)
        return image[..., 3]

    with torch.no_grad():
        target = alpha(torch.tensor([true_offset], device=device))
    offset = torch.zeros(1, device=device, requires_grad=True)
    optimizer = torch.optim.Adam([offset], lr=0.02)
    schedule = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, steps)
    for step in range(steps):
        optimizer.zero_grad()
        loss = torch.mean((alpha(offset) - target) ** 2)
        loss.backward()
        optimizer.step()
        schedule.step()
        if out is not None and step % 10 == 0:
            frame = (alpha(offset).detach()[0].clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
            Image.fromarray(frame).save(os.path.join(out, "frame_%03d.png" % step))
    # world units per pixel in the plane through the cube's centre
    unit = 2.0 * distance * math.tan(math.radians(FOV_Y) / 2.0) / height
    error = abs(float(offset.detach()) - true_offset) / unit
    return {"offset": float(offset.detach()), "true_offset": true_offset, "error_px": error,
            "loss": float(loss.detach())}


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--out", default=None)
    parser.add_argument("--steps", type=int, default=150)
    args = parser.parse_args()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    result = fit(steps=args.steps, out=args.out)
    print("offset %.5f (target %.5f): %.4f px off, loss %.3g" % (
        result["offset"], result["true_offset"], result["error_px"], result["loss"]))


if __name__ == "__main__":
    main()
