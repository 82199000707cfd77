"""Estimate the normals of a scan: K nearest neighbours of every point, then the direction of least variance.

A scan comes without normals; a point-to-plane term, Chamfer with normals or a renderer of the points needs them.
mesh_renderer.points.estimate_point_normals takes every point's K nearest points of the same cloud
(points.knn_points: brute force on the device, a sorted list of K keys per query in registers, no N x N tensor),
forms the neighbourhood's covariance in float64 and returns the eigenvector of its smallest eigenvalue, turned
towards the sensor.

    python examples/estimate_scan_normals.py [--points 5000] [--neighbours 16] [--out normals.xyz]

The cloud is the one fit_mesh_point_cloud.py fits: sampled from a known ellipsoid, so the script needs no data files
and the result can be checked against the ellipsoid's analytic normals.  A single sensor position sees only one side
of a closed surface -- the normals of the far side point inwards by construction -- so the error is the angle between
the two LINES, acos |n . a|.  --out writes one `x y z nx ny nz` line per point.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from fit_mesh_point_cloud import TARGET_SHAPE
from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer import points as point_losses

SENSOR = [0.0, 0.0, 4.0]            # outside the ellipsoid


def ellipsoid_cloud(points=5000, resolution=32, seed=0):
    """`points` float32 host points on the ellipsoid mesh of fit_mesh_point_cloud.py (a sphere of `resolution`
    scaled by TARGET_SHAPE), drawn from a host generator: the same cloud whatever device it is moved to."""
    vertices, triangles, _ = shapes.sphere(1.0, resolution)
    generator = torch.Generator().manual_seed(seed)
    return point_losses.sample_surface_points(vertices * torch.tensor(TARGET_SHAPE), triangles, points,
                                              generator=generator)


def analytic_normals(cloud):
    """The unit normals of the ellipsoid x^2/a^2 + y^2/b^2 + z^2/c^2 = 1 at (the projection of) the points, float64."""
    radii = torch.tensor(TARGET_SHAPE, dtype=torch.float64, device=cloud.device)
    n = cloud.double() / (radii * radii)
    return n / n.norm(dim=-1, keepdim=True)


def angles_to_analytic(cloud, normals):
    """-> (the angle in degrees between every estimated and analytic normal LINE [N], whether the point lies on the
    ellipsoid [N]).  The sphere mesh of common.shapes carries the reference's quirk -- the last triangle of a pole fan
    runs to the other pole, through the interior -- so about one sample in a hundred is not on the surface at all:
    its implicit value x^2/a^2 + y^2/b^2 + z^2/c^2 is far below the facets' 0.98."""
    cosine = (normals.double() * analytic_normals(cloud)).sum(-1).abs().clamp(max=1.0)
    radii = torch.tensor(TARGET_SHAPE, dtype=torch.float64, device=cloud.device)
    return torch.acos(cosine) * (180.0 / math.pi), ((cloud.double() / radii) ** 2).sum(-1) > 0.95


def estimate(points=5000, neighbours=16, device="cuda:0", dtype=torch.float32, out=None, resolution=32, seed=0):
    """-> (mean angle, maximum angle in degrees between the estimated and the analytic normal lines over the whole
    cloud, cloud [N,3], normals [N,3]).  out: a text file of `x y z nx ny nz` lines."""
    cloud = ellipsoid_cloud(points, resolution, seed).to(device=torch.device(device), dtype=dtype)
    sensor = torch.tensor(SENSOR, device=cloud.device, dtype=dtype)
    normals = point_losses.estimate_point_normals(cloud, K=neighbours, orient_to=sensor)
    angles, _ = angles_to_analytic(cloud, normals)
    if out is not None:
        with open(out, "w") as f:
            for p, n in zip(cloud.cpu().tolist(), normals.cpu().tolist()):
                f.write("%.6f %.6f %.6f %.6f %.6f %.6f\n" % tuple(p + n))
    return float(angles.mean()), float(angles.max()), cloud, normals


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--neighbours", type=int, default=16)
    ap.add_argument("--resolution", type=int, default=32)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    mean, worst, cloud, normals = estimate(args.points, args.neighbours, args.device, out=args.out,
                                           resolution=args.resolution)
    facing = int(((normals * (torch.tensor(SENSOR, device=cloud.device) - cloud)).sum(-1) >= 0).sum())
    angles, on_surface = angles_to_analytic(cloud, normals)
    print("%d points, %d neighbours: angle to the analytic normal mean %.3f deg, max %.3f deg (the %d points on the "
          "ellipsoid alone: mean %.3f deg, max %.3f deg); %d normals face the sensor at %s"
          % (cloud.shape[0], args.neighbours, mean, worst, int(on_surface.sum()), float(angles[on_surface].mean()),
             float(angles[on_surface].max()), facing, SENSOR))


if __name__ == "__main__":
    main()
