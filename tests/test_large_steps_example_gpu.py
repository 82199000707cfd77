"""examples/fit_mesh_large_steps.py on the MI355X at tests/test_mesh_point_example_gpu.py's settings: the run is finite
throughout, the .obj has the sphere's vertices, the float64 restatement's two-sided distance
(tests/point_mesh_reference.py + tests/mesh_point_reference.py) of the preconditioned fit to the scan is below the
starting sphere's, and the solves took more than 0 and fewer than max_iterations iterations on average.  Printed,
none asserted: the residual and the mesh terms of the preconditioned fit beside those of plain Adam on the vertices,
and fit_mesh_scan_two_sided.py's 3.3e-4 + 5.8e-5 (its regularised fit at these settings) for comparison.  On the MI355X:
data term 0.0944 -> 3.59e-4 preconditioned, -> 1.61e-4 plain Adam; scan -> mesh + mesh -> scan 5.54e-2 + 3.90e-2 for
the sphere, 3.16e-4 + 3.93e-5 preconditioned, 1.60e-4 + 1.49e-6 plain Adam; mesh terms 0.120 / 0.355 / 0.136
preconditioned against 1.09 / 1.47 / 1.06 for plain Adam; 21.4 conjugate-gradient iterations a solve."""
import importlib.util
import math
import os

import pytest
import torch

import mesh_point_reference as mp
import point_mesh_reference as ref
from conftest import ROOT
from pytorch_mesh_renderer_amd.common import shapes

pytestmark = pytest.mark.gpu


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _vertices_of(path):
    with open(path) as f:
        return torch.tensor([[float(x) for x in line.split()[1:]] for line in f if line.startswith("v ")])


def _two_sided(cloud, vertices, triangles):
    """(point -> mesh mean, mesh -> point mean) of the float64 restatement, one image."""
    p, v = cloud[None], vertices[None]
    to_mesh = ref.mean_of(ref.nearest(p, v, triangles)[0])
    to_points = mp.mean_of(mp.nearest(p, v, triangles)[0], v, triangles)
    return float(to_mesh), float(to_points)


def test_large_steps_example(tmp_path):
    example = _example("fit_mesh_large_steps")
    settings = dict(steps=150, resolution=10, points=2000, device="cuda:0")
    preconditioned, plain = example.optimize(out=str(tmp_path / "large_steps.obj"), **settings)
    for run in (preconditioned, plain):
        assert len(run["losses"]) == 150 and all(math.isfinite(x) for x in run["losses"])
        assert bool(torch.isfinite(run["vertices"]).all()) and bool(torch.isfinite(run["terms"]).all())
    device = torch.device("cuda:0")
    vertices, triangles, _ = shapes.sphere(1.0, 10)
    cloud = example.scan_of(vertices.to(device), triangles.to(device), 2000,
                            torch.Generator(device=device).manual_seed(0)).cpu()
    fitted = _vertices_of(str(tmp_path / "large_steps.obj"))
    assert fitted.shape == vertices.shape and bool(torch.isfinite(fitted).all())
    assert float((fitted - preconditioned["vertices"]).abs().max()) < 1e-5          # (the file's six decimals)
    start = _two_sided(cloud, vertices, triangles)
    end = _two_sided(cloud, fitted, triangles)
    other = _two_sided(cloud, plain["vertices"], triangles)
    print("data term: preconditioned %.6f -> %.6f, plain Adam %.6f -> %.6f" % (
        preconditioned["losses"][0], preconditioned["losses"][-1], plain["losses"][0], plain["losses"][-1]))
    print("float64 residual, scan -> mesh + mesh -> scan: sphere %.3e + %.3e, preconditioned %.3e + %.3e, plain Adam "
          "%.3e + %.3e (fit_mesh_scan_two_sided.py with its regularisers: 3.3e-4 + 5.8e-5)" % (start + end + other))
    print("mesh terms (laplacian, edge length, normal consistency): preconditioned %s, plain Adam %s" % (
        [round(x, 4) for x in preconditioned["terms"].tolist()], [round(x, 4) for x in plain["terms"].tolist()]))
    print("%.1f conjugate-gradient iterations a solve on average" % preconditioned["mean_iterations"])
    assert sum(end) < sum(start)
    assert 0 < preconditioned["mean_iterations"] < preconditioned["max_iterations"]
