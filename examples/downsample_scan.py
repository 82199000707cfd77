"""Thin a scan before fitting to it: farthest-point sampling against a random subset.

Every search in mesh_renderer.points is brute force, so a scan of 10^5 - 10^6 points is thinned before the fitting
loop.  A random subset keeps the sensor's density bias -- dense where the sensor was close, holes elsewhere --
while mesh_renderer.points.sample_farthest_points picks every sample as the point farthest from those picked before
it and so covers the surface evenly.  The script builds a scan of an ellipsoid that is dense near one pole, thins it
both ways and reports the squared covering radius of each subset (the largest squared distance from a scan point to
its nearest sample, points.nearest_points(scan, subset)), then estimates the subset's normals.

    python examples/downsample_scan.py [--points 20000] [--samples 500] [--device cuda:0]

The covering radius of the farthest-point subset is also what sample_farthest_points reports itself: one more sample
is asked for than is kept, and the radius of that last sample is the squared distance of the farthest scan point to
the samples kept.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from fit_mesh_point_cloud import TARGET_SHAPE
from pytorch_mesh_renderer_amd.mesh_renderer import points as point_losses

SENSOR = [0.0, 0.0, 4.0]            # above the pole the scan is dense at
RANDOM_SUBSETS = 3


def scan_cloud(points=20000, seed=0):
    """`points` float32 host points on the ellipsoid with half extents TARGET_SHAPE, from a host generator: the
    longitude uniform, the height z = 1 - 2 u^3 for uniform u, so that half of the points lie above z = 0.75 -- a
    sensor close to the +z pole -- and the far pole is sparse."""
    generator = torch.Generator().manual_seed(seed)
    u = torch.rand(points, 2, generator=generator, dtype=torch.float64)
    z = 1.0 - 2.0 * u[:, 0] ** 3
    ring = (1.0 - z * z).clamp(min=0).sqrt()
    phi = 2.0 * math.pi * u[:, 1]
    unit = torch.stack([ring * torch.cos(phi), ring * torch.sin(phi), z], dim=-1)
    return (unit * torch.tensor(TARGET_SHAPE, dtype=torch.float64)).float()


def covering_radius(scan, subset):
    """The largest squared distance from a point of scan [N,3] to its nearest point of subset [K,3]."""
    return float(point_losses.nearest_points(scan, subset)[0].max())


def downsample(points=20000, samples=500, device="cuda:0", dtype=torch.float32, neighbours=16, seed=0):
    """-> a dict: "scan" [N,3], "subset" [K,3], "idx" [K], "radius" (what sample_farthest_points reports for the
    subset's squared covering radius), "covering" (the same measured by nearest_points), "random" (the measured
    squared covering radii of RANDOM_SUBSETS seeded random subsets of K points), "normals" [K,3] of the subset."""
    scan = scan_cloud(points, seed).to(device=torch.device(device), dtype=dtype)
    samples = min(samples, points - 1)
    _, idx, radius = point_losses.sample_farthest_points(scan, samples + 1, return_radius=True)
    idx = idx[:samples].long()
    subset = scan[idx]
    random = []
    for t in range(RANDOM_SUBSETS):
        pick = torch.randperm(points, generator=torch.Generator().manual_seed(seed + 1 + t))[:samples]
        random.append(covering_radius(scan, scan[pick.to(scan.device)]))
    sensor = torch.tensor(SENSOR, device=scan.device, dtype=dtype)
    normals = point_losses.estimate_point_normals(subset, K=min(neighbours, samples), orient_to=sensor)
    return {"scan": scan, "subset": subset, "idx": idx, "radius": float(radius[samples]),
            "covering": covering_radius(scan, subset), "random": random, "normals": normals}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--neighbours", type=int, default=16)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    out = downsample(args.points, args.samples, args.device, neighbours=args.neighbours)
    print("%d -> %d points: squared covering radius %.3e by farthest-point sampling (it reports %.3e itself), "
          "%s by random subsets; %d of %d normals of the subset are defined"
          % (out["scan"].shape[0], out["subset"].shape[0], out["covering"], out["radius"],
             ", ".join("%.3e" % r for r in out["random"]), int((out["normals"].abs().sum(-1) > 0).sum()),
             out["subset"].shape[0]))


if __name__ == "__main__":
    main()
