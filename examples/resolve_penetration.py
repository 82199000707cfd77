"""Push a mesh out of an obstacle it has sunk into: the signed distance as a penetration penalty.

The package's sphere (radius 0.6, 200 triangles) starts overlapping the package's cube (side 1), shifted so that one
cap of the sphere lies inside it.  An unsigned distance cannot see that: it is small on both sides of the cube's
surface.  mesh_renderer.points.signed_distance is negative inside -- the side comes from the winding number of the
cube around every sphere vertex, the magnitude and the gradient from the exact point-to-mesh distance -- so

    loss = mean(relu(margin - signed_distance(sphere vertices, cube))^2) + mesh_regularizer(sphere)

is zero once every vertex is at least `margin` outside, and its gradient pushes the vertices inside towards the
nearest face of the cube while the regulariser keeps the sphere's triangles well-shaped.

    python examples/resolve_penetration.py [--steps 200] [--margin 0.05] [--out resolved.obj]

Prints the number of sphere vertices inside the cube and the least signed distance, before and after.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer import points as point_losses
from pytorch_mesh_renderer_amd.mesh_renderer import regularizers

CUBE_CENTRE = [0.8, 0.1, 0.05]      # the cube spans x in [0.3, 1.3]: the sphere's +x cap (radius 0.6) is inside


def scene(resolution=10, device="cuda:0"):
    """-> (sphere vertices [V,3], sphere triangles, cube vertices [8,3], cube triangles) on the device."""
    device = torch.device(device)
    vertices, triangles, _ = shapes.sphere(0.6, resolution)
    cube_vertices, cube_triangles, _ = shapes.cube(1.0)
    cube_vertices = cube_vertices + torch.tensor(CUBE_CENTRE)
    return vertices.to(device), triangles.to(device), cube_vertices.to(device), cube_triangles.to(device)


def report(vertices, cube_vertices, cube_triangles):
    """-> (sphere vertices inside the cube, the least signed distance)."""
    with torch.no_grad():
        inside = point_losses.inside_mesh(vertices, cube_vertices, cube_triangles)
        least = point_losses.signed_distance(vertices, cube_vertices, cube_triangles).min()
    return int(inside.sum()), float(least)


def optimize(steps=200, resolution=10, device="cuda:0", out=None, margin=0.05, laplacian=0.02, edge=0.01, normal=0.0,
             lr=0.01):
    """Adam on the sphere's vertices -> (penalty per step, (inside, least signed distance) before, the same after,
    the resolved vertices).  out: a Wavefront .obj file for the resolved sphere."""
    vertices, triangles, cube_vertices, cube_triangles = scene(resolution, device)
    before = report(vertices, cube_vertices, cube_triangles)
    v = vertices.clone().requires_grad_(True)
    optimizer = torch.optim.Adam([v], lr=lr)
    penalties = []
    for _ in range(steps):
        optimizer.zero_grad()
        distance = point_losses.signed_distance(v, cube_vertices, cube_triangles)
        penalty = torch.relu(margin - distance).square().mean()
        loss = penalty + regularizers.mesh_regularizer(v, triangles, laplacian=laplacian, edge=edge, normal=normal)
        loss.backward()
        optimizer.step()
        penalties.append(float(penalty.detach()))
    resolved = v.detach()
    after = report(resolved, cube_vertices, cube_triangles)
    if out is not None:
        with open(out, "w") as f:
            for p in resolved.cpu().tolist():
                f.write("v %.6f %.6f %.6f\n" % tuple(p))
            for t in triangles.cpu().tolist():
                f.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))
    return penalties, before, after, resolved


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--resolution", type=int, default=10)
    ap.add_argument("--margin", type=float, default=0.05)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    penalties, before, after, _ = optimize(args.steps, args.resolution, args.device, args.out, args.margin)
    print("penalty %.6f -> %.6f; sphere vertices inside the cube %d -> %d; least signed distance %.4f -> %.4f"
          % (penalties[0], penalties[-1], before[0], after[0], before[1], after[1]))


if __name__ == "__main__":
    main()
