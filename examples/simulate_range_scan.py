"""Simulate a range scan of a mesh from one sensor position, and register it back: cast_rays as the sensor.

Every other example's "scan" is sample_surface_points over the whole surface.  A real range sensor sees one side of
the object from one position.  Here the cube is moved by a known similarity (12 degrees about (1, 2, 3), a shift,
scale 1.05), a sensor at SENSOR casts a grid of rays at it -- a fan that is wider than the object, so some rays miss --
and the hit points origins + t * directions are the scan: only the three faces the sensor sees.
mesh_renderer.points.iterative_closest_point against the UNMOVED mesh then brings the scan back, and the script
prints the hit count, the scan's root-mean-square distance to the unmoved mesh before and after, and how far the
recovered rotation is from the planted one.  The rotation is determined by the three face normals the sensor sees.  The
scale is not: shrinking the scan about the seen corner keeps every point on its plane, so any scale at or below the
planted one leaves no residual -- what a one-view scan cannot tell, the script prints beside the planted value.

    python examples/simulate_range_scan.py [--grid 96] [--iterations 40] [--device cuda:0]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer import points as point_ops

AXIS, DEGREES, SHIFT, SCALE = (1.0, 2.0, 3.0), 12.0, (0.1, -0.05, 0.08), 1.05
SENSOR, FAN = (4.0, 3.0, 3.5), 0.42   # the sensor's position, and half the fan's opening as a tangent


def rotation(axis, degrees):
    """[3,3] float64 for row vectors: p @ rotation turns p by `degrees` about `axis`."""
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    t = math.radians(degrees)
    return (torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1.0 - math.cos(t)) * K @ K).T


def sensor_rays(grid, target):
    """A grid x grid fan of rays from SENSOR around the direction to `target` [3] -> (origins, directions) [grid^2,3]
    float64; the directions are not normalised."""
    eye = torch.tensor(SENSOR, dtype=torch.float64)
    forward = target - eye
    forward = forward / forward.norm()
    right = torch.linalg.cross(forward, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
    right = right / right.norm()
    up = torch.linalg.cross(right, forward)
    steps = (torch.arange(grid, dtype=torch.float64) + 0.5) / grid * 2.0 - 1.0
    u, v = torch.meshgrid(steps, steps, indexing="ij")
    directions = forward + FAN * (u[..., None] * right + v[..., None] * up)
    return eye.expand(grid * grid, 3).contiguous(), directions.reshape(-1, 3)


def rms_distance(scan, vertices, triangles):
    """The root of the mean squared distance from the points to the mesh."""
    return float(point_ops.nearest_triangles(scan, vertices, triangles)[0].mean().sqrt())


def angle_between(R_a, R_b):
    """The angle in degrees of the rotation that takes R_a to R_b."""
    d = R_a.double().cpu().T @ R_b.double().cpu()
    sine = torch.stack([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]]).norm() / 2.0
    return math.degrees(math.atan2(float(sine), (float(d.trace()) - 1.0) / 2.0))


def simulate(grid=96, iterations=40, device="cuda:0", dtype=torch.float32):
    """-> a dict: "origins", "directions", "moved" (the moved vertices), "triangles", "t", "face", "scan" (the hit
    points), "hits" and "rays" (counts), "before" and "after" (the scan's rms distance to the unmoved mesh), "angle"
    (degrees between the recovered and the planted rotation) and "solution" (the ICPSolution)."""
    dev = torch.device(device)
    vertices, triangles, _ = shapes.cube(2.0)
    R, T = rotation(AXIS, DEGREES), torch.tensor(SHIFT, dtype=torch.float64)
    moved = SCALE * vertices.double() @ R + T
    origins, directions = sensor_rays(grid, moved.mean(0))
    origins, directions = origins.to(dev, dtype), directions.to(dev, dtype)
    moved, still, triangles = moved.to(dev, dtype), vertices.to(dev, dtype), triangles.to(dev)
    t, face, _ = point_ops.cast_rays(origins, directions, moved, triangles)
    hit = face >= 0
    scan = (origins + t[:, None] * directions)[hit]                      # a one-view scan of the moved cube
    before = rms_distance(scan, still, triangles)
    solution = point_ops.iterative_closest_point(scan, (still, triangles), max_iterations=iterations,
                                                 estimate_scale=True, relative_rmse_thr=0.0)
    after = rms_distance(solution.Xt, still, triangles)
    # the scan lies on SCALE * cube @ R + T, so s * scan @ R' + T' ~ cube wants R' = R^T
    return {"origins": origins, "directions": directions, "moved": moved, "triangles": triangles, "t": t, "face": face,
            "scan": scan, "hits": int(hit.sum()), "rays": int(hit.numel()), "before": before, "after": after,
            "angle": angle_between(solution.RTs.R, R.T), "solution": solution}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", type=int, default=96)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    out = simulate(args.grid, args.iterations, args.device)
    print("%d of %d rays hit; faces seen: %s" % (out["hits"], out["rays"],
                                                  sorted(set(out["face"][out["face"] >= 0].tolist()))))
    print("rms distance of the scan to the unmoved mesh: %.4e before, %.4e after %d rounds of ICP"
          % (out["before"], out["after"], int(out["solution"].iterations)))
    print("recovered rotation is %.3f degrees from the planted one; scale %.4f (planted 1 / %.2f = %.4f: one view of "
          "three planes bounds it from above only)"
          % (out["angle"], float(out["solution"].RTs.s), SCALE, 1.0 / SCALE))


if __name__ == "__main__":
    main()
