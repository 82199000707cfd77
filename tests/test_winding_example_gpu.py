"""examples/resolve_penetration.py on the MI355X at small settings: the signed distance as a penetration penalty pushes
the sphere's cap out of the cube.  Checked with the float64 restatement on the CPU (tests/winding_reference.py: the
winding number of the cube around every sphere vertex, and the analytic signed distance to the box): some vertices
start inside, none end inside, and the final least signed distance is not negative.  The same settings through the
torch route on the CPU: 20 -> 0 vertices inside, least signed distance -0.2648 -> 0.0891."""
import importlib.util
import os

import pytest
import torch

import winding_reference as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _truth(vertices, cube_vertices, cube_triangles, centre):
    """-> (vertices inside the cube by the float64 winding number, the least float64 signed distance to the box)."""
    w, _ = ref.winding(vertices.cpu()[None], cube_vertices.cpu()[None], cube_triangles.cpu())
    exact = ref.box_signed_distance(vertices.cpu().double() - torch.tensor(centre, dtype=torch.float64))
    assert torch.equal(w[0] >= 0.5, exact < 0)   # the two float64 statements agree on every vertex
    return int((w[0] >= 0.5).sum()), float(exact.min())


def test_resolve_penetration_example(tmp_path):
    example = _example("resolve_penetration")
    penalties, before, after, resolved = example.optimize(steps=80, device="cuda:0", out=str(tmp_path / "resolved.obj"))
    print("penalty %.6f -> %.6f; inside %d -> %d; least signed distance %.4f -> %.4f"
          % (penalties[0], penalties[-1], before[0], after[0], before[1], after[1]))
    start, _, cube_vertices, cube_triangles = example.scene(device="cpu")
    inside_before, least_before = _truth(start, cube_vertices, cube_triangles, example.CUBE_CENTRE)
    inside_after, least_after = _truth(resolved, cube_vertices, cube_triangles, example.CUBE_CENTRE)
    assert len(penalties) == 80 and penalties[-1] < 1e-3 * penalties[0]
    assert inside_before > 0 and least_before < 0
    assert inside_after == 0 and least_after >= 0
    # what the example itself printed agrees with the float64 truth
    assert before[0] == inside_before and after[0] == 0
    assert abs(before[1] - least_before) < 1e-5 and abs(after[1] - least_after) < 1e-5
    assert os.path.getsize(str(tmp_path / "resolved.obj")) > 0
