"""Deform a sphere until its silhouettes match four target views with the HARD rasterizer, kept usable by the
mesh regularisers.

render(..., antialias=True) gives the binary alpha of the hard rasterizer a gradient to the outline's vertices and
to those only; mesh_renderer.regularizers.mesh_regularizer (uniform Laplacian + edge length + normal consistency,
one forward and one backward launch on the device) spreads the motion over the surface and keeps the triangles
well-shaped.  The soft-rasterizer counterpart with the regularisers spelled in eager torch is
fit_mesh_silhouettes.py.

    python examples/fit_mesh_regularized.py --out /tmp/frames [--steps 200]

The targets are rendered from a known ellipsoid, so the script needs no data files and the result can be checked.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from PIL import Image

from pytorch_mesh_renderer_amd import mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer import regularizers

TARGET_SHAPE = [0.65, 1.0, 0.8]     # half extents of the ellipsoid to recover
EYES = [[0.0, 0.0, -3.0], [3.0, 0.0, 0.0], [-3.0, 0.0, 0.0], [0.0, 0.0, 3.0]]


def optimize(steps=200, size=96, resolution=12, laplacian=0.1, edge=0.05, normal=0.02, lr=0.01, device="cuda:0",
             out=None):
    """Adam on the sphere's vertices: silhouette MSE over the four views + the weighted regularisers (a weight of 0
    switches its term off).  -> (silhouette loss per step, half extents [3] of the fitted mesh, its final
    mesh_terms [3] = (Laplacian, edge length, normal consistency))."""
    device = torch.device(device)
    vertices, triangles, normals = shapes.sphere(1.0, resolution)
    vertices, triangles = vertices.to(device), triangles.to(device)
    B = len(EYES)
    eye = torch.tensor(EYES, device=device)
    center = torch.zeros_like(eye)
    up = torch.tensor([[0.0, 1.0, 0.0]] * B, device=device)
    # alpha does not depend on the shading: constant normals, one light at each camera
    normals = normals.to(device).unsqueeze(0).repeat(B, 1, 1)
    diffuse = torch.ones(B, vertices.shape[0], 3, device=device)
    light_positions = eye.unsqueeze(1)
    light_intensities = torch.ones(B, 1, 3, device=device)

    def render(v):
        return mesh_renderer.render(v.unsqueeze(0).expand(B, -1, -1).contiguous(), triangles, normals, diffuse, eye,
                                    center, up, light_positions, light_intensities, size, size, fov_y=60.0,
                                    antialias=True)

    with torch.no_grad():
        target_alpha = render(vertices * torch.tensor(TARGET_SHAPE, device=device))[..., 3]
    v = vertices.clone().requires_grad_(True)
    optimizer = torch.optim.Adam([v], lr=lr)
    losses = []
    for step in range(steps):
        optimizer.zero_grad()
        image = render(v)
        silhouette = torch.mean((image[..., 3] - target_alpha) ** 2)
        loss = silhouette + regularizers.mesh_regularizer(v, triangles, laplacian=laplacian, edge=edge, normal=normal)
        loss.backward()
        optimizer.step()
        losses.append(float(silhouette.detach()))
        if out is not None and step % 20 == 0:
            frame = torch.cat(list(image[..., 3].detach().clamp(0, 1)), dim=1)
            Image.fromarray((frame * 255).to(torch.uint8).cpu().numpy()).save(os.path.join(out, "fit_%04d.png" % step))
    fitted = v.detach()
    extent = (fitted.max(0).values - fitted.min(0).values).cpu() / 2.0
    return losses, extent, regularizers.mesh_terms(fitted, triangles)[0].cpu()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    losses, extent, terms = optimize(args.steps, out=args.out)
    print("silhouette loss %.5f -> %.5f; half extents %s (target %s); laplacian %.4f, edge length %.4f, normal "
          "consistency %.4f" % (losses[0], losses[-1], [round(x, 3) for x in extent.tolist()], TARGET_SHAPE,
                                float(terms[0]), float(terms[1]), float(terms[2])))


if __name__ == "__main__":
    main()
