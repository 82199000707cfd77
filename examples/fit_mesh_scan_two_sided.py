"""Deform a sphere until its surface matches a scan with the exact distance in BOTH directions: point_mesh_face_distance
+ the mesh regularisers, no rendering and no sampling.

fit_mesh_scan.py measures every scan point against the nearest triangle exactly, but keeps a sampled one-directional
Chamfer term for the other half, which brings back the noise floor of the sample spacing and a gradient that jitters
with the samples.  Here that half is exact too: mesh_renderer.points.mesh_point_distance measures every triangle
against the nearest scan point, so parts of the mesh that no scan point is near are still pulled in, and
point_mesh_face_distance is the sum of the two means.  Nothing in the loop draws random numbers: the same start gives
the same fit, bit for bit.

    python examples/fit_mesh_scan_two_sided.py [--steps 300] [--points 5000] [--out fitted.obj]

The cloud is fit_mesh_scan.py's: sampled once from a known ellipsoid, so the script needs no data files and the
result can be checked.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from fit_mesh_scan import TARGET_SHAPE, scan_of
from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer import points as point_losses
from pytorch_mesh_renderer_amd.mesh_renderer import regularizers


def optimize(steps=300, resolution=16, points=5000, device="cuda:0", out=None, laplacian=0.1, edge=0.05, normal=0.01,
             lr=0.01, seed=0):
    """Adam on the sphere's vertices: point_mesh_face_distance(cloud, mesh) + the weighted regularisers.
    -> (data term per step, half extents [3] of the fitted mesh, its final mesh_terms [3]).  out: a Wavefront .obj
    file for the fitted mesh."""
    device = torch.device(device)
    vertices, triangles, _ = shapes.sphere(1.0, resolution)
    vertices, triangles = vertices.to(device), triangles.to(device)
    generator = torch.Generator(device=device).manual_seed(seed)
    cloud = scan_of(vertices, triangles, points, generator)
    v = vertices.clone().requires_grad_(True)
    optimizer = torch.optim.Adam([v], lr=lr)
    losses = []
    for _ in range(steps):
        optimizer.zero_grad()
        data = point_losses.point_mesh_face_distance(cloud, v, triangles)
        loss = data + regularizers.mesh_regularizer(v, triangles, laplacian=laplacian, edge=edge, normal=normal)
        loss.backward()
        optimizer.step()
        losses.append(float(data.detach()))
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
    print("data term %.6f -> %.6f; half extents %s (target %s); laplacian %.4f, edge length %.4f, normal consistency "
          "%.4f" % (losses[0], losses[-1], [round(x, 3) for x in extent.tolist()], TARGET_SHAPE, float(terms[0]),
                    float(terms[1]), float(terms[2])))


if __name__ == "__main__":
    main()
