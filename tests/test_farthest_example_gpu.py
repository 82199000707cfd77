"""examples/downsample_scan.py on the MI355X: a scan of 20 000 points, dense near one pole, thinned to 500.

Only the ordering is asserted: the farthest-point subset covers the scan within a smaller radius than each of the
three seeded random subsets (on the host torch path it does by 6.5x to 10x).  What sample_farthest_points reports as
the subset's squared covering radius -- the radius of one sample more -- must be the one nearest_points measures:
both are the float32 squared distance of the same pair of points, one un-fused and one with the compiler's
contraction, each within 4 * 2^-24 of the true value, hence 1e-6 relative."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _example():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("downsample_scan", os.path.join(root, "examples", "downsample_scan.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    return example


def test_downsample_scan_example():
    out = _example().downsample(points=20000, samples=500, device="cuda:0")
    print("covering %.4e (reported %.4e), random %s" % (out["covering"], out["radius"], out["random"]))
    assert out["scan"].is_cuda and out["subset"].shape == (500, 3) and out["normals"].shape == (500, 3)
    assert len(out["random"]) == 3
    for random in out["random"]:
        assert out["covering"] < random
    assert abs(out["radius"] - out["covering"]) <= 1e-6 * out["covering"]
    assert int(out["idx"].unique().numel()) == 500
    lengths = out["normals"].norm(dim=-1)
    assert bool(((lengths - 1).abs() < 1e-4).all())
    assert bool(torch.isfinite(out["normals"]).all())
