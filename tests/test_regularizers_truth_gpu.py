"""reg.mesh_terms on the MI355X (csrc/mesh_reg.hip), forward and backward, against the float64 truth of
tests/mesh_regularizer_truth.py: every value within its a-posteriori bound, every vertex's gradient within its own
E_v, no vertex exempt; translated meshes, nearly flat grids, slivers and every launch edge of the kernels.  The
bounds, their constants and the caps are derived in mesh_regularizer_truth.py and measured on the CPU in
test_regularizers_truth_host.py.

WORST MEASURED err/E of the kernels on the MI355X (2026-10-21), values (lap / edge / nc) and per-vertex gradient, over
every run of the cases:
  sphere20 at the four offsets     0.078 / 0.067 / 0.163    gradient 0.174      (restatement 0.074 / 0.145 / 0.174, 0.204)
  sphere50 at the four offsets     0.012 / 0.072 / 0.037    gradient 0.204      (0.012 / 0.115 / 0.029, 0.106)
  grid_1e-1 .. grid_1e-4           0.029 / 0.108 / 0.047    gradient 0.254      (0.014 / 0.079 / 0.047, 0.086)
  grid_planar                      -     / 0.007 / 0.041    gradient 0.172      (nc: exactly 0 in float64)
  sliver (1:256)                   -     / 0.084 / 0.007    gradient 0.032      (- / 0.057 / 0.003, 0.033)
  strips V = 1 .. 65               0.131 / 0.098 / 0.240    gradient 0.206      (0.133 / 0.109 / 0.182, 0.184)
  flaps_255, _256, _257            0.081 / 0.046 / 0.195    gradient 0.209      (0.070 / 0.046 / 0.195, 0.099)
  grid_91 (354 and 95 rows)        0.045 / 0.007 / 0.006    gradient 0.174      (0.045 / 0.075 / 0.006, 0.152)
  fans, valence 7, 8, 9, 16, 17    0.103 / 0.159 / 0.094    gradient 0.150      (0.099 / 0.073 / 0.086, 0.065)
  subsets (dterms with 0 and < 0)  0.078 / 0.047 / 0.163    gradient 0.193      (0.053 / 0.145 / 0.134, 0.140)
In brackets the float32 restatement on the CPU (<= 1/4 by the choice of the constants).  The share of vertices with
E_v <= 1e-4 max|grad| (or the run's own decade in mesh_regularizer_truth.CAPS) is >= 0.974 in every run, 1.000 in all
but the sliver's and the grids' runs with the Laplacian.  The Laplacian's value on the grids flatter than 1e-1, which
runs at OFFSET too, sits at 0.006 .. 0.020 of E_lap.
flap_gradient is unchanged: on the flat grids (the normal term alone or with the edge term) the kernel's worst
gradient err/E is 0.254, 0.175, 0.219 and 0.186 for sigma = 1e-1 .. 1e-4, 2 to 4 times the float32 autograd of the stable
form (0.064, 0.060, 0.086, 0.052) and a factor of 4 inside E_v.
THE KERNELS BEFORE THIS SUITE (delta_i = (1/deg) sum v_j - v_i, nc = 1 - cos) failed 15 of these cases on the MI355X
(2026-10-21; worst err/E up to each test's first failing run).  Laplacian gradient, sphere20 at offset 0 / 10 / 100 /
1000: 1.09 / 8.3 / 38.8 / 310 (value 14.3 at 1000); sphere50: 1.05 / 12.1 / 113 / 35.8 (value 8.7 at 1000); grid_1e-1
at OFFSET 418 (value 3.6); subsets 125.  Normal-consistency value: grid_1e-3 24.3 and 15.1 (at OFFSET), grid_1e-4 358,
and the fans of valence 8 and 17, 2.36 and 1.007.  Every other case of that run passed, the launch edges included
(the grids ran without the Laplacian then, and the sliver was another one).
"""
import pytest
import torch

import mesh_regularizer_truth as truth
from pytorch_mesh_renderer_amd import _native, mesh_renderer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
reg = mesh_renderer.regularizers


def _run(vertices, triangles, dterms, **kwargs):
    leaf = vertices.to(DEV).requires_grad_(True)
    got = reg.mesh_terms(leaf, triangles, **kwargs)
    assert got.shape == (vertices.shape[0], 3) and got.dtype == torch.float32 and got.is_cuda
    got.backward(dterms.float().to(DEV))
    return got.detach(), leaf.grad


@pytest.mark.parametrize("name", truth.CASES)
def test_mesh_terms_match_the_truth(name):
    c = truth.case(name)
    tri = c.triangles.to(DEV)
    if name == "grid_91":   # the second trip of the row sum, asserted here so that the case cannot stop covering it
        V, F = c.topo["V"], len(c.topo["flaps"])
        assert truth.forward_rows(V, F, True, True, True) > truth.ROWS_PER_TRIP
        assert truth.forward_rows(V, F, False, False, True) == -(-F // truth.FLAPS_PER_BLOCK)
    if name.startswith("flaps_"):
        assert len(c.topo["flaps"]) == int(name[6:]) == reg.mesh_topology(tri, c.topo["V"]).flap_count
    for run in c.runs:
        got, grad = _run(c.vertices, tri, c.dterms, **run)
        truth.check(got, grad, truth.truth_of(name, run), "%s %s kernel" % (name, truth.run_key(run)),
                    *truth.caps_of(name, run))
        for k, on in enumerate((run["laplacian"], run["edge"], run["normal"])):
            if not on:
                assert bool((got[:, k] == 0).all())


@pytest.mark.parametrize("mesh", ["sphere20", "sphere50"])
def test_a_batch_of_the_four_offsets_equals_its_single_images(mesh):
    cases = [truth.case("%s@%s" % (mesh, at)) for at in truth.OFFSETS]
    tri = cases[0].triangles.to(DEV)
    vertices = torch.cat([c.vertices[:1] for c in cases])
    dterms = torch.cat([c.dterms[:1] for c in cases])
    for target in (None, 0.05):
        got, grad = _run(vertices, tri, dterms, target_length=target)
        for b in range(len(cases)):
            alone, alone_grad = _run(vertices[b:b + 1], tri, dterms[b:b + 1], target_length=target)
            assert torch.equal(alone[0], got[b]), "image %d: its terms depend on the rest of the batch" % b
            assert torch.equal(alone_grad[0], grad[b])


@pytest.mark.parametrize("name", ["sphere20@100", "grid_1e-3@0"])
def test_repeats_and_the_deterministic_mode_are_bit_identical(name):
    c = truth.case(name)
    tri = c.triangles.to(DEV)
    before = _native.set_deterministic(False)
    try:
        runs = []
        for mode in (False, False, True, True):
            _native.set_deterministic(mode)
            runs.append(_run(c.vertices, tri, c.dterms, **c.runs[0]))
    finally:
        _native.set_deterministic(before)
    for got, grad in runs[1:]:
        assert torch.equal(got, runs[0][0]) and torch.equal(grad, runs[0][1])
