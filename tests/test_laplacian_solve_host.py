"""mesh_renderer.preconditioning without a GPU: the operator against a float64 matrix built from the triangles' sides
(tests/laplacian_solve_reference.py), the torch route of the solve against the certified truth, the freeze rules,
the bit-for-bit properties, the argument errors, the C ABI's refusals -- and the accuracy of the float32
restatement cg32, from which the device tests' bound is made."""
import ctypes

import numpy as np
import pytest
import torch

import laplacian_solve_reference as lref
from pytorch_mesh_renderer_amd import _native, mesh_renderer

pre = mesh_renderer.preconditioning
OPERATOR_MESHES = ("sphere8", "sphere25", "strip7", "strip200", "fan300", "strays")


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


@pytest.mark.parametrize("kind", OPERATOR_MESHES)
@pytest.mark.parametrize("lam", [0.0, 0.37, 19.0])
def test_to_differential_is_the_matrix_of_the_triangles_sides(kind, lam):
    vertices, triangles = lref.tensors(kind)
    V = vertices.shape[0]
    x = torch.from_numpy(np.random.default_rng(V).standard_normal((2, V, 4)))
    want = np.stack([lref.system64(kind, lam) @ x[b].numpy() for b in range(2)])
    got = pre.to_differential(x, triangles, lam)
    assert got.dtype == torch.float64 and got.shape == x.shape
    assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    assert torch.equal(pre.to_differential(x[1], triangles.long(), lam), got[1])          # [V,C], any integer dtype
    dense = lref.system64(kind, lam).dense()
    assert np.array_equal(dense, dense.T) and np.abs(dense @ x[0].numpy() - want[0]).max() <= 1e-11 * np.abs(want).max()
    if kind == "strays":                                                                   # the identity rows
        assert torch.equal(got[:, -2:], x[:, -2:])


@pytest.mark.parametrize("kind", ["sphere8", "sphere25", "fan300", "strays"])
def test_float64_route_solves_to_the_truth(kind):
    _, triangles = lref.tensors(kind)
    for lam in lref.LAMBDAS:
        b = lref.batch(kind, 3).astype(np.float64)
        x64 = lref.truth(kind, lam, b)
        for tol in (1e-6, 1e-9):
            x, iterations, residual = pre.from_differential(torch.from_numpy(b), triangles, lam, tol=tol,
                                                            return_info=True)
            assert x.dtype == torch.float64 and iterations.dtype == torch.int32 and residual.dtype == torch.float32
            assert iterations.shape == residual.shape == (3, 3)
            error = lref.relative_error(x.numpy(), x64, b)
            # |x - x*| <= |b - A x| <= tol |b| for the recurrence's residual; the true one drifts from it by at most
            # u |A| iterations = 1.1e-16 x 6e4 (the fan at lam = 100) x 150 < 1e-9 in float64
            assert error.max() <= tol + 1e-9, (lam, tol, error.max())
            assert int(iterations.max()) < 300 and float(residual.max()) <= tol * (1 + 1e-6)
            assert int(iterations.min()) >= (1 if lam == 0 else 2)


def test_gradcheck_of_both_functions():
    vertices, triangles = lref.tensors("sphere8")
    x = vertices.double().clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: pre.to_differential(t, triangles, 3.0), (x,))
    u = pre.to_differential(vertices.double(), triangles, 3.0).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: pre.from_differential(t, triangles, 3.0, tol=1e-13), (u,),
                                    atol=1e-7, rtol=1e-6)
    start = vertices.double().clone().requires_grad_(True)
    x, iterations, residual = pre.from_differential(u, triangles, 3.0, tol=1e-13, x0=start, return_info=True)
    assert not iterations.requires_grad and not residual.requires_grad
    x.sum().backward()
    assert start.grad is None and u.grad is not None                                       # x0 receives no gradient


def test_the_solve_is_symmetric():
    _, triangles = lref.tensors("sphere25")
    rng = np.random.default_rng(5)
    b, y = (torch.from_numpy(rng.standard_normal((627, 2))) for _ in range(2))
    sb, sy = (pre.from_differential(t, triangles, 19.0, tol=1e-12) for t in (b, y))
    left, right = float((y * sb).sum()), float((sy * b).sum())
    assert abs(left - right) <= 1e-10 * max(abs(left), 1.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_freeze_rules(dtype):
    _, triangles = lref.tensors("sphere8")
    b = torch.from_numpy(lref.batch("sphere8", 2)).to(dtype)
    # rule 1 before the first iteration: b = 0 gives x = 0 exactly, 0 iterations, residual 0
    zero = b.clone()
    zero[1] = 0
    x, iterations, residual = pre.from_differential(zero, triangles, 19.0, return_info=True)
    assert bool((x[1] == 0).all()) and iterations[1].tolist() == [0, 0] and residual[1].tolist() == [0.0, 0.0]
    clean = pre.from_differential(b, triangles, 19.0, return_info=True)
    assert _bits(x[0], clean[0][0]) and _bits(x[2], clean[0][2])
    # rule 2: a NaN in one system makes THAT system NaN, 0 iterations; every other system keeps its bits
    bad = b.clone()
    bad[1, 17, 0] = float("nan")
    x, iterations, residual = pre.from_differential(bad, triangles, 19.0, return_info=True)
    assert bool(torch.isnan(x[1, :, 0]).all()) and int(iterations[1, 0]) == 0 and bool(torch.isnan(residual[1, 0]))
    assert _bits(x[1, :, 1], clean[0][1, :, 1]) and _bits(x[0], clean[0][0]) and _bits(x[2], clean[0][2])
    assert torch.equal(iterations[0], clean[1][0]) and torch.equal(iterations[2], clean[1][2])
    bad[1, 17, 0] = float("inf")
    assert bool(torch.isnan(pre.from_differential(bad, triangles, 19.0)[1, :, 0]).all())
    # tol = 0: a system runs until r = 0 exactly, breakdown (rule 3) or the last iteration, and stays finite
    x, iterations, residual = pre.from_differential(b, triangles, 19.0, tol=0.0, max_iterations=600, return_info=True)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(residual).all())
    assert 0 < int(iterations.min()) and int(iterations.max()) <= 600
    x64 = lref.truth("sphere8", 19.0, b.numpy())
    assert lref.relative_error(x.numpy(), x64, b.numpy()).max() <= (1e-5 if dtype == torch.float32 else 1e-13)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_bit_for_bit_properties(dtype):
    _, triangles = lref.tensors("sphere25")
    b = torch.from_numpy(lref.batch("sphere25", 3)).to(dtype)
    whole = pre.from_differential(b, triangles, 19.0, return_info=True)
    again = pre.from_differential(b, triangles, 19.0, return_info=True)
    assert all(_bits(p, q) for p, q in zip(whole, again))
    started = pre.from_differential(b, triangles, 19.0, x0=torch.zeros_like(b), return_info=True)
    assert all(_bits(p, q) for p, q in zip(whole, started))
    for k in range(3):                                       # a batch equals its singles
        one = pre.from_differential(b[k:k + 1], triangles, 19.0, return_info=True)
        assert all(_bits(p[0], q[k]) for p, q in zip(one, whole))
        single = pre.from_differential(b[k], triangles, 19.0, return_info=True)
        assert single[0].shape == (627, 3) and single[1].shape == single[2].shape == (3,)
        assert all(_bits(p, q[k]) for p, q in zip(single, whole))
    assert len(set(whole[1].max(dim=1).values.tolist())) > 1  # (the images froze at different iterations)
    M = int(whole[1].min()) + 2
    short = pre.from_differential(b, triangles, 19.0, max_iterations=M, return_info=True)
    longer = pre.from_differential(b, triangles, 19.0, max_iterations=M + 64, return_info=True)
    frozen = short[1] < M
    assert bool(frozen.any()) and not bool(frozen.all())
    assert _bits(short[0].transpose(1, 2)[frozen], longer[0].transpose(1, 2)[frozen])
    assert torch.equal(short[1][frozen], longer[1][frozen]) and _bits(short[2][frozen], longer[2][frozen])
    assert bool((short[1][~frozen] == M).all())
    # a warm start is a start: from the solution only its own rounding is left to remove
    warm = pre.from_differential(b, triangles, 19.0, x0=whole[0], return_info=True)
    assert bool((warm[1] < whole[1]).all()) and int(warm[1].max()) <= 8


def test_no_iterations():
    _, triangles = lref.tensors("sphere8")
    b = torch.from_numpy(lref.batch("sphere8", 3))
    x, iterations, residual = pre.from_differential(b, triangles, 19.0, max_iterations=0, return_info=True)
    assert bool((x == 0).all()) and bool((iterations == 0).all()) and bool((residual == 1).all())
    start = torch.from_numpy(np.random.default_rng(2).standard_normal(b.shape).astype(np.float32))
    x, iterations, _ = pre.from_differential(b, triangles, 19.0, max_iterations=0, x0=start, return_info=True)
    assert _bits(x, start) and bool((iterations == 0).all())


def test_argument_errors():
    vertices, triangles = lref.tensors("sphere8")
    b = vertices.clone()
    for call in (pre.to_differential, pre.from_differential):
        with pytest.raises(TypeError):
            call(b.numpy(), triangles, 1.0)
        with pytest.raises(TypeError):
            call(b.long(), triangles, 1.0)
        with pytest.raises(TypeError):
            call(b, triangles, torch.tensor(1.0))
        with pytest.raises(TypeError):
            call(b, triangles.numpy(), 1.0)
        with pytest.raises(RuntimeError):
            call(b, triangles.float(), 1.0)
        with pytest.raises(ValueError):
            call(b, triangles[:, :2], 1.0)
        with pytest.raises(ValueError):
            call(b[:, 0], triangles, 1.0)
        with pytest.raises(ValueError):
            call(torch.zeros(1, 66, 5), triangles, 1.0)      # C > 4
        with pytest.raises(ValueError):
            call(torch.zeros(1, 0, 3), triangles, 1.0)
        for lam in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                call(b, triangles, lam)
    for bad in (dict(tol=-1e-6), dict(tol=float("nan")), dict(max_iterations=-1), dict(max_iterations=10001),
                dict(check_every=-1), dict(x0=torch.zeros(65, 3)), dict(x0=torch.zeros(66, 3, dtype=torch.float64))):
        with pytest.raises(ValueError):
            pre.from_differential(b, triangles, 1.0, **bad)
    for bad in (dict(tol="1e-6"), dict(max_iterations=3.0), dict(check_every=None), dict(x0=np.zeros((66, 3)))):
        with pytest.raises(TypeError):
            pre.from_differential(b, triangles, 1.0, **bad)
    assert pre.from_differential(b, triangles, 1.0, max_iterations=10000).shape == b.shape


def test_native_wrappers_refuse_before_the_library():
    vertices, triangles = lref.tensors("sphere8")
    topology = _native.mesh_topology(triangles, 66)
    b = vertices[None].contiguous()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.laplacian_apply(b, topology, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.laplacian_solve(b, topology, 1.0)
    with pytest.raises(ValueError):
        _native.laplacian_apply(b, _native.mesh_topology(triangles, 67), 1.0)         # another vertex count
    with pytest.raises(ValueError):
        _native.laplacian_solve(b, (topology.nbr_offsets, topology.nbr), 1.0)         # not a MeshTopology
    with pytest.raises(RuntimeError):
        _native.laplacian_solve(b.double(), topology, 1.0)
    with pytest.raises(ValueError):
        _native.laplacian_solve(b[0], topology, 1.0)
    with pytest.raises(ValueError):
        _native.laplacian_solve(torch.zeros(1, 66, 5), topology, 1.0)
    for bad in (dict(lam=-1.0), dict(lam=float("nan")), dict(tol=-1.0), dict(max_iterations=10001),
                dict(max_iterations=-1), dict(check_every=-2), dict(route=3), dict(x0=torch.zeros(1, 66, 2))):
        with pytest.raises(ValueError):
            _native.laplacian_solve(b, topology, **{"lam": 1.0, **bad})


def test_abi_entries_refuse_bad_arguments_without_a_device():
    L = _native.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)     # (never dereferenced: every call below is refused)
    EINVAL = _native.MR_EINVAL
    out = (ctypes.c_int * 4)()
    outs = [ctypes.c_void_p(ctypes.addressof(out) + 4 * k) for k in range(4)]

    def apply(x=one, offsets=one, nbr=one, B=1, V=66, C=3, nnz=384, lam=1.0, y=one):
        return L.mr_laplacian_apply(x, offsets, nbr, B, V, C, nnz, lam, y, null)

    for bad in (dict(x=null), dict(y=null), dict(offsets=null), dict(nbr=null), dict(B=0), dict(B=65536), dict(V=0),
                dict(V=1 << 28), dict(C=0), dict(C=5), dict(nnz=-1), dict(lam=-1.0), dict(lam=float("nan")),
                dict(lam=float("inf"))):
        assert apply(**bad) == EINVAL, bad

    def solve(b=one, x0=null, offsets=one, nbr=one, B=1, V=66, C=3, nnz=384, lam=1.0, tol=1e-6, max_iterations=300,
              route=0, first=0, count=300, x=one, iterations=one, residual=one, ws=one, ws_bytes=1 << 30):
        return L.mr_laplacian_solve(b, x0, offsets, nbr, B, V, C, nnz, lam, tol, max_iterations, route, first, count,
                                    null, x, iterations, residual, ws, ws_bytes, null)

    for bad in (dict(b=null), dict(x=null), dict(iterations=null), dict(residual=null), dict(offsets=null),
                dict(nbr=null), dict(B=0), dict(V=0), dict(V=1 << 28), dict(C=5), dict(nnz=-1), dict(lam=-0.5),
                dict(lam=float("nan")), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")),
                dict(max_iterations=-1), dict(max_iterations=10001), dict(route=3), dict(route=-1), dict(first=-1),
                dict(first=301), dict(count=-1), dict(V=4000, route=1)):
        assert solve(**bad) == EINVAL, bad
    assert solve(ws=null) == _native.MR_EWORKSPACE and solve(ws_bytes=16) == _native.MR_EWORKSPACE
    assert solve(ws=ctypes.c_void_p(264)) == _native.MR_EWORKSPACE                        # misaligned
    assert L.mr_laplacian_solve_workspace_bytes(0, 66, 3) == 0 == L.mr_laplacian_solve_workspace_bytes(1, 66, 5)
    # five planes, and the partials and states on top
    assert L.mr_laplacian_solve_workspace_bytes(32, 2502, 3) >= 5 * 32 * 2502 * 3 * 4
    for bad in ((0, 3, 0), (1 << 28, 3, 0), (66, 0, 0), (66, 5, 0), (66, 3, 3), (3073, 3, 1)):
        assert L.mr_laplacian_solve_plan(*bad, *outs) == EINVAL, bad
    assert L.mr_laplacian_solve_plan(66, 3, 0, null, *outs[1:]) == EINVAL
    assert L.mr_laplacian_solve_plan(66, 3, 0, *outs) == _native.MR_OK


def test_the_plan_needs_no_gpu_and_depends_on_v_and_c_alone():
    small = _native.laplacian_solve_plan(66, 3)
    assert small == {"route": 1, "workgroup_size": 64, "vertices_per_lane": 2}
    assert _native.laplacian_solve_plan(2502, 3)["route"] == 1
    assert _native.laplacian_solve_plan(100000, 3)["route"] == 2
    assert _native.laplacian_solve_plan(66, 3, route=_native.LAPLACIAN_ROUTE_STEPS)["route"] == 2
    last = max(V for V in range(1, 1 << 14) if _native.laplacian_solve_plan(V, 4)["route"] == 1)
    with pytest.raises(ValueError):
        _native.laplacian_solve_plan(last + 1, 4, route=_native.LAPLACIAN_ROUTE_RESIDENT)
    for C in (1, 2, 3, 4):                                   # p in LDS: 4 C bytes a vertex, within the 160 KB of a CU
        resident = _native.laplacian_solve_plan(last, C)
        assert resident["route"] == 1 and last * 4 * C <= 160 * 1024
        assert resident["workgroup_size"] * resident["vertices_per_lane"] >= last
    for bad in ((0, 3), (66, 0), (66, 5), (1 << 28, 3)):
        with pytest.raises(ValueError):
            _native.laplacian_solve_plan(*bad)


def test_accuracy_of_the_float32_restatement():
    """cg32's own error |x32 - x64| / |b| for every case the device tests use (their bound is max(tol, 4 x this)), and
    its iteration counts: printed as the table of tests/laplacian_solve_reference.py's docstring.  Asserted: the
    restatement converges well inside max_iterations, and its error stays below 1e-4 -- |x - x*| <= |b - A x|, and
    the TRUE residual of a float32 recurrence floors at 1e-5 to 8e-5 |b| on these systems whatever tol asks for."""
    print("\n    mesh      lam   smooth    noise     delta     iterations")
    for kind in lref.MESHES:
        for lam in lref.LAMBDAS:
            errors = np.zeros(3)
            most = 0
            for C in lref.CHANNELS:
                case = lref.case(kind, lam, C)
                errors = np.maximum(errors, case["cg32_error"].max(axis=1))
                most = max(most, int(case["cg32_iterations"].max()))
                assert case["cg32_iterations"].max() < 150, (kind, lam, C)
                assert case["cg32_error"].max() <= 1e-4, (kind, lam, C)
            print("    %-8s %4g   %-9.2g %-9.2g %-9.2g %3d" % ((kind, lam) + tuple(errors) + (most,)))
            if lam == 0:
                assert most == 1 and errors.max() == 0
