"""examples/fit_mesh_point_cloud.py on the MI355X: surface sampling + Chamfer distance + the regularisers fit a sphere
to a cloud sampled from an ellipsoid."""
import importlib.util
import os

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_point_cloud_fit_example():
    spec = importlib.util.spec_from_file_location("fit_mesh_point_cloud",
                                                  os.path.join(ROOT, "examples", "fit_mesh_point_cloud.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    losses, extent, terms = example.optimize(steps=150, resolution=10, points=2000, device="cuda:0", out=None)
    print("chamfer %.6f -> %.6f, half extents %s, terms %s" % (losses[0], losses[-1], extent.tolist(), terms.tolist()))
    assert len(losses) == 150
    assert losses[-1] < 0.3 * losses[0]
    target = example.TARGET_SHAPE[0]
    assert float(extent[0]) < 1.0 and abs(float(extent[0]) - target) < 0.5 * abs(1.0 - target)
