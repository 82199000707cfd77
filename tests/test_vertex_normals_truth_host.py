"""The meshes of tests/vertex_normals_reference.py are fit to judge the vertex-normal kernels by (no GPU needed): no
vertex sits where float32 and float64 could take different branches of the normalisation, the cases hold what their
names say.
"""
import pytest
import torch

import vertex_normals_reference as vr


@pytest.mark.parametrize("name", vr.NAMES)
def test_no_vertex_sum_is_near_the_eps_of_the_normalisation(name):
    """|sum| is either exactly zero, in both precisions, or clear of eps = 1e-6 by a factor of ten each way."""
    c = vr.case(name)
    for run in (c.truth, c.f32):
        length = run["sums"].double().norm(dim=2)
        zero = (run["sums"] == 0).all(2)
        assert not bool(((length >= 1e-7) & (length <= 1e-5)).any()), name
        assert bool((zero | (length > 1e-5)).all()), name
    assert torch.equal((c.truth["sums"] == 0).all(2), (c.f32["sums"] == 0).all(2))
    for k in ("normals", "d_vertices"):
        assert bool(torch.isfinite(c.truth[k]).all()) and bool(torch.isfinite(c.f32[k]).all())


@pytest.mark.parametrize("n", vr.FAN_VALENCES)
def test_fans_have_the_hub_valence_they_name(n):
    c = vr.case("fan-%d" % n)
    assert int((c.triangles == 0).sum()) == n and c.vertices.shape == (2, n + 2, 3)
    assert float(c.truth["d_vertices"][:, 0].abs().min()) > 0.0


@pytest.mark.parametrize("V", vr.SIZES)
def test_sizes(V):
    c = vr.case("size-%d" % V)
    assert c.vertices.shape == (2, V, 3)
    if V >= 3:
        assert c.triangles.shape == (2 * V, 3) and float(c.truth["d_vertices"].abs().max()) > 0.0
    else:
        assert not bool(c.truth["normals"].any()) and not bool(c.truth["d_vertices"].any())


def test_zero_area_case_takes_the_eps_branch_and_leaves_the_isolated_vertices_alone():
    c = vr.case("zero-area")
    z, iso = c.groups["zero-area"], c.groups["isolated"]
    assert torch.equal(c.vertices[:, z[1]], c.vertices[:, z[2]]) and not torch.equal(c.vertices[:, z[0]], c.vertices[:, z[1]])
    for run in (c.truth, c.f32):
        assert not bool(run["sums"][:, z + iso].any()) and not bool(run["normals"][:, z + iso].any())
        assert not bool(run["d_vertices"][:, iso].any())
    # d normal / d sum = 1 / eps on the three vertices: gradients of the order of 1e6 times the triangle's edge
    assert float(c.truth["d_vertices"][:, z].abs().max()) > 1e5
    assert c.r["zero-area", "d_vertices"] < 1e-5
    touching = [t for t in c.triangles.tolist() if set(t) & set(z)]
    assert touching == [z]


def test_repeated_id_and_out_of_range_cases_hold_them():
    c = vr.case("repeated-id")
    assert any(t[0] == t[1] != t[2] for t in c.triangles.tolist())
    c = vr.case("out-of-range")
    V = c.vertices.shape[1]
    bad = [i for i, t in enumerate(c.triangles.tolist()) if min(t) < 0 or max(t) >= V]
    assert len(bad) == 2 and bad[0] not in (0, len(c.triangles) - 1)
    keep = [i for i in range(len(c.triangles)) if i not in bad]
    without = vr.run(c.vertices, c.triangles[keep], c.weights, torch.float64)
    assert torch.equal(without["d_vertices"], c.truth["d_vertices"]) and torch.equal(without["normals"], c.truth["normals"])

