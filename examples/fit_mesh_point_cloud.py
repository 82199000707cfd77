"""Deform a sphere until its surface matches a point cloud: Chamfer distance + the mesh regularisers, no rendering.

The data term for fitting a mesh to 3D data (a scan, a depth camera's points, another mesh).  Every step samples the
CURRENT mesh's surface (mesh_renderer.points.sample_surface_points: area-weighted, differentiable to the vertices),
compares the samples with the cloud (points.chamfer_distance: brute-force nearest neighbours in both directions on
the device, no N x M tensor) and adds regularizers.mesh_regularizer, which keeps the triangles well-shaped while the
data term pulls.  The image-driven counterpart is fit_mesh_regularized.py.

    python examples/fit_mesh_point_cloud.py [--steps 300] [--points 5000] [--out fitted.obj]

The cloud is sampled once from a known ellipsoid, so the script needs no data files and the result can be checked.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer import points as point_losses
from pytorch_mesh_renderer_amd.mesh_renderer import regularizers

TARGET_SHAPE = [0.55, 1.0, 0.8]     # half extents of the ellipsoid the cloud is sampled from


def optimize(steps=300, resolution=16, points=5000, device="cuda:0", out=None, laplacian=0.1, edge=0.05, normal=0.01,
             lr=0.01, seed=0):
    """Adam on the sphere's vertices: chamfer_distance(samples of the mesh, cloud) + the weighted regularisers.
    -> (Chamfer term per step, half extents [3] of the fitted mesh, its final mesh_terms [3]).  out: a Wavefront
    .obj file for the fitted mesh."""
    device = torch.device(device)
    vertices, triangles, _ = shapes.sphere(1.0, resolution)
    vertices, triangles = vertices.to(device), triangles.to(device)
    generator = torch.Generator(device=device).manual_seed(seed)
    with torch.no_grad():
        ellipsoid = vertices * torch.tensor(TARGET_SHAPE, device=device)
        cloud = point_losses.sample_surface_points(ellipsoid, triangles, points, generator=generator)
    v = vertices.clone().requires_grad_(True)
    optimizer = torch.optim.Adam([v], lr=lr)
    losses = []
    for _ in range(steps):
        optimizer.zero_grad()
        samples = point_losses.sample_surface_points(v, triangles, points, generator=generator)
        chamfer = point_losses.chamfer_distance(samples, cloud)
        loss = chamfer + regularizers.mesh_regularizer(v, triangles, laplacian=laplacian, edge=edge, normal=normal)
        loss.backward()
        optimizer.step()
        losses.append(float(chamfer.detach()))
    fitted = v.detach()
    if out is not None:
        with open(out, "w") as f:
            for p in fitted.cpu().tolist():
                f.write("v %.6f %.6f %.6f\n" % tuple(p))
            for t in triangles.cpu().tolist():
                f.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))
    extent = (fitted.max(0).values - fitted.min(0).values).cpu() / 2.0
    return losses, extent, regularizers.mesh_terms(fitted, triangles)[0].cpu()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    losses, extent, terms = optimize(args.steps, args.resolution, args.points, args.device, args.out)
    print("chamfer %.6f -> %.6f; half extents %s (target %s); laplacian %.4f, edge length %.4f, normal consistency "
          "%.4f" % (losses[0], losses[-1], [round(x, 3) for x in extent.tolist()], TARGET_SHAPE, float(terms[0]),
                    float(terms[1]), float(terms[2])))


if __name__ == "__main__":
    main()
