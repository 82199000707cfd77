"""examples/simulate_range_scan.py on the MI355X at small settings: a 48 x 48 fan of rays from one sensor position at
the moved cube, the hit points registered back to the unmoved cube with iterative_closest_point.

The fan is wider than the cube, so it has hits and misses.  Every hit point o + t d is held to the moved mesh in
float64 (tests/point_mesh_reference.py): its exact distance is at most |d| E_t + 4 x 2^-24 (|o| + t |d|) -- E_t the
restatement's bound on t at the face the kernel named (tests/ray_reference.py), the rest the float32 rounding of t d and
of the sum.  ICP's residual must end below its start.  The recovered rotation is printed, not asserted beyond that:
through the float32 torch route on the host the same settings give 689 hits of 2304 rays, an rms distance of 1.55e-01
before and 8.3e-06 after 40 rounds, and a rotation 0.001 degrees from the planted one."""
import importlib.util
import os

import pytest
import torch

import point_mesh_reference as pm
import ray_reference as ref

pytestmark = pytest.mark.gpu


def _example():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("simulate_range_scan",
                                                  os.path.join(root, "examples", "simulate_range_scan.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    return example


def test_simulate_range_scan_example(device="cuda:0"):
    out = _example().simulate(grid=48, iterations=40, device=device)
    print("%d of %d rays hit; rms %.4e -> %.4e; rotation %.4f degrees from the planted one, scale %.4f"
          % (out["hits"], out["rays"], out["before"], out["after"], out["angle"], float(out["solution"].RTs.s)))
    assert out["rays"] == 48 * 48 and 0 < out["hits"] < out["rays"]
    o, d, v, tri = (out[k].cpu() for k in ("origins", "directions", "moved", "triangles"))
    t, face = out["t"].cpu(), out["face"].cpu()
    hit = face >= 0
    assert out["scan"].shape == (out["hits"], 3) and bool(torch.isfinite(out["scan"]).all())
    q = ref.evaluate(o[None], d[None], v[None], tri)
    Et = torch.gather(q.Et[0], 1, face.clamp(min=0).long()[:, None])[:, 0]
    bound = d.double().norm(dim=-1) * Et + 4 * ref.EPS * (o.double().norm(dim=-1) + t.double() * d.double().norm(dim=-1))
    exact, _ = pm.nearest(out["scan"].cpu()[None], v[None], tri)
    distance = exact[0].sqrt()
    print("worst distance of a hit point to the moved mesh %.3g, worst distance / bound %.3f, largest bound %.3g"
          % (float(distance.max()), float((distance / bound[hit]).max()), float(bound[hit].max())))
    assert float(bound[hit].max()) < ref.EASY_BOUND   # the bound stays tight: scan points lie 5 to 7 units from the sensor
    assert bool((distance <= bound[hit]).all())
    assert out["after"] < out["before"]
