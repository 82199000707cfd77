"""Deform a sphere until its surface matches a scan with NO regulariser: Laplacian preconditioning keeps the mesh
usable instead (Nicolet, Jacobson, Jakob: "Large Steps in Inverse Rendering", 2021).

fit_mesh_scan_two_sided.py adds a weighted sum of three regularisers to the data term; the penalty that keeps the
mesh from tangling also stops it short of the data, and its weights are tuned per scene.  Here the data term
point_mesh_face_distance stands alone.  The optimiser does not move the vertices x but u = (I + lam L) x, and every
step recovers x = (I + lam L)^-1 u with mesh_renderer.preconditioning.from_differential, a conjugate-gradient solve
on the device started from the previous step's vertices.  The gradient that reaches the vertices has passed through
that inverse: it is smooth by construction.  For comparison the same loss is also run with plain Adam on the
vertices, which has nothing to keep the surface smooth.

    python examples/fit_mesh_large_steps.py [--steps 300] [--points 5000] [--lam 19] [--out fitted.obj]

The problem is fit_mesh_scan_two_sided.py's: the same scan of a known ellipsoid, the same sphere, the same steps.
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
from pytorch_mesh_renderer_amd.mesh_renderer import preconditioning, regularizers


def _write_obj(path, vertices, triangles):
    with open(path, "w") as f:
        for p in vertices.cpu().tolist():
            f.write("v %.6f %.6f %.6f\n" % tuple(p))
        for t in triangles.cpu().tolist():
            f.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))


def optimize(steps=300, resolution=16, points=5000, device="cuda:0", out=None, lam=19.0, lr=0.1, tol=1e-6,
             max_iterations=300, seed=0):
    """Adam on u = (I + lam L) x with the data term alone, and the same loss with Adam on the vertices themselves,
    both at the learning rate lr -- ten times the other fitting examples' 0.01 by default: the large step is what the
    parametrisation is for (at 0.01 it smooths just as well and gets less far in the same steps).
    -> (preconditioned, plain): two dicts with "losses" (the data term per step), "terms" (mesh_terms [3] of the
    final mesh) and "vertices" [V,3]; the preconditioned one also has "mean_iterations" of the solves and
    "max_iterations".  out: a Wavefront .obj file for the preconditioned mesh."""
    device = torch.device(device)
    vertices, triangles, _ = shapes.sphere(1.0, resolution)
    vertices, triangles = vertices.to(device), triangles.to(device)
    generator = torch.Generator(device=device).manual_seed(seed)
    cloud = scan_of(vertices, triangles, points, generator)

    u = preconditioning.to_differential(vertices, triangles, lam).requires_grad_(True)
    optimizer = torch.optim.Adam([u], lr=lr)
    previous, losses, iterations = vertices, [], torch.zeros((), device=device)
    for _ in range(steps):
        optimizer.zero_grad()
        x, solve_iterations, _ = preconditioning.from_differential(u, triangles, lam, tol=tol, x0=previous,
                                                                   max_iterations=max_iterations, return_info=True)
        data = point_losses.point_mesh_face_distance(cloud, x, triangles)
        data.backward()
        optimizer.step()
        previous = x.detach()
        losses.append(float(data.detach()))
        iterations += solve_iterations.float().mean()
    fitted = preconditioning.from_differential(u.detach(), triangles, lam, tol=tol, x0=previous,
                                               max_iterations=max_iterations)
    preconditioned = dict(losses=losses, vertices=fitted.cpu(), terms=regularizers.mesh_terms(fitted, triangles)[0].cpu(),
                          mean_iterations=float(iterations) / max(steps, 1), max_iterations=max_iterations)

    v = vertices.clone().requires_grad_(True)
    optimizer = torch.optim.Adam([v], lr=lr)
    losses = []
    for _ in range(steps):
        optimizer.zero_grad()
        data = point_losses.point_mesh_face_distance(cloud, v, triangles)
        data.backward()
        optimizer.step()
        losses.append(float(data.detach()))
    plain = dict(losses=losses, vertices=v.detach().cpu(), terms=regularizers.mesh_terms(v.detach(), triangles)[0].cpu())
    if out is not None:
        _write_obj(out, fitted, triangles)
    return preconditioned, plain


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--lam", type=float, default=19.0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    preconditioned, plain = optimize(args.steps, args.resolution, args.points, args.device, args.out, lam=args.lam)
    for name, run in (("preconditioned", preconditioned), ("plain Adam", plain)):
        extent = (run["vertices"].max(0).values - run["vertices"].min(0).values) / 2.0
        print("%-14s data term %.6f -> %.6f; half extents %s (target %s); laplacian %.4f, edge length %.4f, normal "
              "consistency %.4f" % (name, run["losses"][0], run["losses"][-1], [round(x, 3) for x in extent.tolist()],
                                    TARGET_SHAPE, float(run["terms"][0]), float(run["terms"][1]),
                                    float(run["terms"][2])))
    print("%.1f conjugate-gradient iterations a solve on average (at most %d)"
          % (preconditioned["mean_iterations"], preconditioned["max_iterations"]))


if __name__ == "__main__":
    main()
