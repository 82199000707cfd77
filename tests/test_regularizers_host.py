"""Mesh regularisers without a GPU: the topology, closed forms, the float64 restatement against finite differences,
the package's host torch path against the restatement, argument refusals and the C ABI's validation."""
import ctypes
import importlib.util
import itertools
import os

import pytest
import torch

import mesh_regularizer_reference as ref
from conftest import ROOT
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

reg = mesh_renderer.regularizers


def _meshes():
    out = {"sphere%d" % k: shapes.sphere(1.0, k)[:2] for k in (4, 6, 12)}
    out["cube"] = shapes.cube(2.0)[:2]
    out["odd"] = ref.odd_mesh()
    return out


MESHES = _meshes()


def _csr(offsets, entries):
    offsets, entries = offsets.tolist(), entries.tolist()
    return [entries[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


@pytest.mark.parametrize("name", sorted(MESHES))
def test_topology_matches_the_loops(name):
    vertices, triangles = MESHES[name]
    V = vertices.shape[0]
    topo = reg.mesh_topology(triangles.clone(), V)
    want = ref.topology(triangles, V)
    assert (topo.vertex_count, topo.edge_count, topo.flap_count) == (V, len(want["edges"]), len(want["flaps"]))
    for t in topo.tensors():
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert [tuple(e) for e in topo.edges.tolist()] == want["edges"]
    assert _csr(topo.nbr_offsets, topo.nbr) == [want["neighbours"][v] for v in range(V)]
    assert [tuple(f) for f in topo.flaps.tolist()] == want["flaps"]
    # the inverse index: every (flap, role) exactly once, at the vertex that has the role, ascending
    flaps = topo.flaps.tolist()
    seen = []
    for v, entries in enumerate(_csr(topo.role_offsets, topo.roles)):
        assert entries == sorted(entries)
        for entry in entries:
            assert flaps[entry // 4][entry % 4] == v
        seen += entries
    assert sorted(seen) == list(range(4 * len(flaps)))


def test_sphere_and_odd_mesh_counts():
    for k, (V, E, F, valence) in {6: (38, 111, 105, None), 12: (146, 435, 429, 16)}.items():
        vertices, triangles = MESHES["sphere%d" % k]
        topo = reg.mesh_topology(triangles, vertices.shape[0])
        assert (topo.vertex_count, topo.edge_count, topo.flap_count) == (V, E, F)
        if valence:
            assert int((topo.nbr_offsets[1:] - topo.nbr_offsets[:-1]).max()) == valence
    for k in (4, 6, 12):   # the seam and pole quirk of shapes.sphere
        vertices, triangles = MESHES["sphere%d" % k]
        want = ref.topology(triangles, vertices.shape[0])
        assert len(want["boundary"]) == 6 and not want["nonmanifold"]
    vertices, triangles = ref.odd_mesh()
    want = ref.topology(triangles, 10)
    assert (0, 1, 2, 3) in want["flaps"] and (1, 2) in want["nonmanifold"] and want["boundary"]
    assert want["neighbours"][9] == [] and (4, 5) in want["edges"] and not any(f[:2] == (4, 5) for f in want["flaps"])
    assert all(max(e) < 10 for e in want["edges"])
    assert (2, 6, 7, 7) in want["flaps"] and (6, 8) in want["edges"] and (3, 5, 8, 0) in want["flaps"]
    assert bool((vertices[6] == vertices[8]).all())


def test_topology_is_cached_on_the_tensor():
    vertices, triangles = shapes.sphere(1.0, 4)[:2]
    first = reg.mesh_topology(triangles, vertices.shape[0])
    assert reg.mesh_topology(triangles, vertices.shape[0]) is first
    assert reg.mesh_topology(triangles, vertices.shape[0] + 1) is not first
    wide = triangles.long()
    assert reg.mesh_topology(wide, vertices.shape[0]) is reg.mesh_topology(wide, vertices.shape[0])
    triangles[0, 0] = triangles[0, 0]            # an in-place write moves the version counter
    assert reg.mesh_topology(triangles, vertices.shape[0]) is not first
    empty = reg.mesh_topology(torch.zeros(0, 3, dtype=torch.int64), 5)
    assert (empty.edge_count, empty.flap_count) == (0, 0) and empty.nbr_offsets.tolist() == [0] * 6


def test_closed_forms():
    square = torch.tensor([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=torch.float64)
    for second in ([0, 2, 3], [0, 3, 2]):        # both windings of the second triangle
        triangles = torch.tensor([[0, 1, 2], second])
        assert float(reg.normal_consistency(square, triangles)) == 0.0
        assert float(ref.terms(square[None], ref.topology(triangles, 4))[0, 2]) == 0.0
    folded = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, 1, 0]], dtype=torch.float64)
    triangles = torch.tensor([[0, 1, 2], [1, 0, 3]])
    assert abs(float(reg.normal_consistency(folded, triangles)) - 2.0) < 1e-15
    assert abs(float(ref.terms(folded[None], ref.topology(triangles, 4))[0, 2]) - 2.0) < 1e-15
    # a regular unit-edge mesh: the tetrahedron
    tetra = torch.tensor([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=torch.float64) / 8 ** 0.5
    triangles = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    assert abs(float(reg.edge_length(tetra, triangles)) - 1.0) < 1e-15
    assert abs(float(reg.edge_length(tetra, triangles, target_length=1.0))) < 1e-30
    batch = torch.stack([tetra, 2.0 * tetra])
    assert torch.allclose(reg.edge_length(batch, triangles, target_length=1.0), torch.tensor([0.0, 1.0]).double())
    # no edges, no flaps: zeros; a lone vertex contributes no Laplacian
    none = torch.zeros(0, 3, dtype=torch.int32)
    assert reg.mesh_terms(tetra, none).tolist() == [[0.0, 0.0, 0.0]]


SUBSETS = [s for s in itertools.product((False, True), repeat=3)]


def test_restatement_gradients_match_finite_differences():
    for name, target in (("sphere4", None), ("odd", 0.7)):
        vertices, triangles = MESHES[name]
        g = torch.Generator().manual_seed(5)
        v = (vertices.double() + 0.05 * torch.randn(vertices.shape, generator=g, dtype=torch.float64))[None]
        topo = ref.topology(triangles, v.shape[1])
        dterms = torch.tensor([[0.7, -1.3, 0.9]], dtype=torch.float64)
        _, grad = ref.gradients(v, topo, dterms, target_length=target)
        h = 1e-6
        worst = 0.0
        for i in range(v.shape[1]):
            for k in range(3):
                plus, minus = v.clone(), v.clone()
                plus[0, i, k] += h
                minus[0, i, k] -= h
                fd = ((ref.terms(plus, topo, target_length=target) - ref.terms(minus, topo, target_length=target))
                      * dterms).sum() / (2 * h)
                worst = max(worst, abs(float(fd) - float(grad[0, i, k])))
        # central differences of a smooth function: O(h^2) truncation + 1e-16 / h rounding, both below 1e-8 here
        assert worst < 1e-7 * max(1.0, float(grad.abs().max())), (name, worst)


@pytest.mark.parametrize("name", ["sphere6", "odd", "cube"])
def test_host_path_matches_the_restatement(name):
    vertices, triangles = MESHES[name]
    B = 2
    g = torch.Generator().manual_seed(11)
    v = vertices[None].repeat(B, 1, 1).double()
    if name != "odd":                            # the odd mesh keeps its exact degeneracies
        v = v + 0.05 * torch.randn(v.shape, generator=g, dtype=torch.float64)
    dterms = torch.randn(B, 3, generator=g, dtype=torch.float64)
    topo = ref.topology(triangles, v.shape[1])
    for (lap, edge, normal), target in itertools.product(SUBSETS, (None, 0.4)):
        kwargs = dict(laplacian=lap, edge=edge, normal=normal, target_length=target)
        want, want_grad = ref.gradients(v, topo, dterms, **kwargs)
        leaf = v.clone().requires_grad_(True)
        got = reg.mesh_terms(leaf, triangles, **kwargs)
        assert got.dtype == torch.float64 and got.shape == (B, 3)
        assert float((got.detach() - want).abs().max()) <= 1e-12
        if lap or edge or normal:
            (got * dterms).sum().backward()
            assert bool(torch.isfinite(leaf.grad).all())
            assert float((leaf.grad - want_grad).abs().max()) <= 1e-12
    # float32 host tensors take the same path
    got32 = reg.mesh_terms(v.float(), triangles)
    assert got32.dtype == torch.float32
    assert float((got32.double() - ref.terms(v, topo)).abs().max()) <= 1e-5


def test_single_terms_and_weighted_sum():
    vertices, triangles = ref.perturbed_sphere(6, 2, seed=3)
    v = vertices.double()
    all_terms = reg.mesh_terms(v, triangles)
    assert torch.equal(reg.laplacian_smoothing(v, triangles), all_terms[:, 0])
    assert torch.equal(reg.edge_length(v, triangles), all_terms[:, 1])
    assert torch.equal(reg.normal_consistency(v, triangles), all_terms[:, 2])
    assert reg.laplacian_smoothing(v[0], triangles).dim() == 0
    assert torch.equal(reg.edge_length(v[1], triangles.long(), target_length=0.3),
                       reg.mesh_terms(v, triangles, target_length=0.3)[1, 1])
    total = reg.mesh_regularizer(v, triangles, laplacian=0.5, edge=0.0, normal=2.0)
    assert torch.allclose(total, 0.5 * all_terms[:, 0] + 2.0 * all_terms[:, 2], rtol=1e-14, atol=0)
    assert reg.mesh_regularizer(v[0], triangles, edge=1.0).dim() == 0
    assert reg.mesh_regularizer(v, triangles).tolist() == [0.0, 0.0]
    strided = torch.zeros(2, v.shape[1], 6, dtype=torch.float64)
    strided[..., ::2] = v
    assert torch.equal(reg.mesh_terms(strided[..., ::2], triangles), all_terms)


def test_argument_refusals():
    vertices, triangles = shapes.sphere(1.0, 4)[:2]
    for bad in (triangles.float(), triangles.bool(), triangles.double()):
        with pytest.raises(RuntimeError, match="triangles must hold integer vertex indices"):
            reg.mesh_terms(vertices, bad)
        with pytest.raises(RuntimeError, match="triangles must hold integer vertex indices"):
            reg.mesh_topology(bad, vertices.shape[0])
    with pytest.raises(ValueError):
        reg.mesh_terms(vertices[:, :2], triangles)
    with pytest.raises(ValueError):
        reg.mesh_terms(vertices[None, None], triangles)
    with pytest.raises(ValueError):
        reg.mesh_terms(vertices, triangles[:, :2])
    with pytest.raises(TypeError):
        reg.mesh_terms(vertices.long(), triangles)
    with pytest.raises(TypeError):
        reg.mesh_terms(vertices, triangles.tolist())
    # the device wrappers refuse host tensors: the torch path above is not a fallback for them
    topo = reg.mesh_topology(triangles, vertices.shape[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.mesh_regularizer_forward(vertices[None], topo, 7)
    with pytest.raises(ValueError):
        _native.mesh_regularizer_forward(vertices[None, :-1], topo, 7)
    with pytest.raises(ValueError):
        _native.mesh_regularizer_forward(vertices[None], topo, 8)


def test_abi_validates_before_touching_a_device():
    L = _native.lib()
    null = ctypes.c_void_p(0)
    some = ctypes.c_void_p(256)                  # never dereferenced: every call below is refused first
    query = L.mr_mesh_regularizer_workspace_bytes
    assert query(0, 10, 10) == 0 and query(-1, 10, 10) == 0 and query(1, 0, 10) == 0 and query(1, 10, -1) == 0
    assert query(70000, 10, 10) == 0
    need = query(32, 2502, 7500)                 # one row of three floats per workgroup
    assert need >= 32 * ((2502 + 31) // 32 + (7500 + 255) // 256) * 12 and need % 256 == 0
    assert query(1, 1, 0) > 0
    fwd, bwd = L.mr_mesh_regularizer_forward, L.mr_mesh_regularizer_backward
    EINVAL = _native.MR_EINVAL

    def forward(vertices=some, offsets=some, nbr=some, flaps=some, B=1, V=8, E=12, F=6, terms=7, unit=some, out=some,
                ws=some, ws_bytes=1 << 20):
        return fwd(vertices, offsets, nbr, flaps, B, V, E, F, terms, 0, 0.0, unit, out, ws, ws_bytes, null)

    def backward(dterms=some, vertices=some, unit=some, offsets=some, nbr=some, flaps=some, role_offsets=some,
                 roles=some, B=1, V=8, E=12, F=6, terms=7, out=some):
        return bwd(dterms, vertices, unit, offsets, nbr, flaps, role_offsets, roles, B, V, E, F, terms, 0, 0.0, out,
                   null)

    for kwargs in (dict(vertices=null), dict(offsets=null), dict(nbr=null), dict(flaps=null), dict(unit=null),
                   dict(out=null), dict(B=0), dict(B=-3), dict(B=65536), dict(V=0), dict(V=-1), dict(E=-1),
                   dict(F=-1), dict(terms=8), dict(terms=-1)):
        assert forward(**kwargs) == EINVAL, kwargs
    assert forward(ws=null) == _native.MR_EWORKSPACE
    assert forward(ws_bytes=8) == _native.MR_EWORKSPACE
    assert forward(ws=ctypes.c_void_p(264)) == _native.MR_EWORKSPACE
    for kwargs in (dict(dterms=null), dict(vertices=null), dict(unit=null), dict(offsets=null), dict(nbr=null),
                   dict(flaps=null), dict(role_offsets=null), dict(roles=null), dict(out=null), dict(B=0), dict(V=0),
                   dict(E=-1), dict(F=-1), dict(terms=9)):
        assert backward(**kwargs) == EINVAL, kwargs


def _load_example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_values_equal_the_fitting_examples_own_functions():
    example = _load_example("fit_mesh_silhouettes")
    vertices, triangles = ref.perturbed_sphere(10, 1, seed=2)
    v = vertices[0].double()
    edges = example.compute_edges_list(triangles)
    laplacian = example.compute_laplacian(v.shape[0], edges).double()
    want_lap = float(example.mesh_laplacian_smoothing_loss(v, laplacian))
    want_edge = float(example.mesh_edge_loss(v, edges))
    # the example builds its 1 / degree weights in float32: 6e-8 relative each
    assert abs(float(reg.laplacian_smoothing(v, triangles)) - want_lap) <= 1e-6 * want_lap
    assert abs(float(reg.edge_length(v, triangles)) - want_edge) <= 1e-12 * want_edge
    topo = ref.topology(triangles, v.shape[0])
    got = ref.terms(v[None], topo)[0]
    assert abs(float(got[0]) - want_lap) <= 1e-6 * want_lap and abs(float(got[1]) - want_edge) <= 1e-12 * want_edge
