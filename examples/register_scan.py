"""Bring a scan into the mesh's frame before fitting to it: ICP against the mesh itself, and against sampled points.

Every loss of mesh_renderer.points, and every fit_mesh_*.py here, assumes that the scan already lies in the mesh's
frame; their basin of attraction is about one sample spacing.  A real scan arrives in the sensor's frame: rotated,
shifted, often at another scale.  The script samples a scan on the cube, moves it by a known similarity (12 degrees
about (1, 2, 3), a shift, scale 1.05) and registers it back with mesh_renderer.points.iterative_closest_point --
once against the mesh (the match of a point is its closest point on the nearest triangle) and once against the same
number of points sampled on the mesh.  Against samples ICP stalls at the sampling noise; against the surface itself
it keeps improving, which is why the mesh target exists.

    python examples/register_scan.py [--points 2000] [--iterations 30] [--device cuda:0]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer import points as point_losses

AXIS, DEGREES, SHIFT, SCALE = (1.0, 2.0, 3.0), 12.0, (0.1, -0.05, 0.08), 1.05


def rotation(axis, degrees):
    """[3,3] float64 for row vectors: p @ rotation turns p by `degrees` about `axis`."""
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    t = math.radians(degrees)
    return (torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1.0 - math.cos(t)) * K @ K).T


def errors(transform, R, T, s):
    """(angle in degrees, shift, relative scale) between a SimilarityTransform and the planted (R, T, s)."""
    d = transform.R.double().cpu().T @ R
    sine = torch.stack([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]]).norm() / 2.0
    angle = math.degrees(math.atan2(float(sine), (float(d.trace()) - 1.0) / 2.0))
    return angle, float((transform.T.double().cpu() - T).norm()), abs(float(transform.s) / s - 1.0)


def optimize(points=2000, iterations=30, device="cuda:0", dtype=torch.float32, seed=0):
    """-> a dict: "mesh" and "sampled", each (angle error in degrees, shift error, relative scale error) of the
    registration against that target, "rmse" of both, and the two ICPSolutions."""
    dev = torch.device(device)
    vertices, triangles, _ = shapes.cube(2.0)
    generator = torch.Generator().manual_seed(seed)
    on_mesh = point_losses.sample_surface_points(vertices.double(), triangles, points, generator=generator)
    sampled = point_losses.sample_surface_points(vertices.double(), triangles, points, generator=generator)
    R, T = rotation(AXIS, DEGREES), torch.tensor(SHIFT, dtype=torch.float64)
    scan = ((on_mesh - T) @ R.T / SCALE).to(device=dev, dtype=dtype)       # SCALE * scan @ R + T lies on the cube
    settings = dict(max_iterations=iterations, estimate_scale=True, relative_rmse_thr=0.0)
    to_mesh = point_losses.iterative_closest_point(scan, (vertices.to(dev, dtype), triangles.to(dev)), **settings)
    to_samples = point_losses.iterative_closest_point(scan, sampled.to(dev, dtype), **settings)
    return {"mesh": errors(to_mesh.RTs, R, T, SCALE), "sampled": errors(to_samples.RTs, R, T, SCALE),
            "rmse": (float(to_mesh.rmse), float(to_samples.rmse)), "solutions": (to_mesh, to_samples)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    out = optimize(args.points, args.iterations, args.device)
    for name, rmse, solution in zip(("mesh", "sampled"), out["rmse"], out["solutions"]):
        angle, shift, scale = out[name]
        print("%-7s target: angle error %.3e deg, shift error %.3e, scale error %.3e, rmse %.3e after %d rounds%s"
              % (name, angle, shift, scale, rmse, int(solution.iterations), "" if bool(solution.converged)
                 else " (not converged)"))


if __name__ == "__main__":
    main()
