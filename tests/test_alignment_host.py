"""corresponding_points_alignment and iterative_closest_point without a GPU: the torch spelling in float64 against
the numpy restatement (tests/alignment_reference.py) to 1e-12, every option and every degenerate case of the
interface, argument errors, gradcheck, the C ABI's size checks -- and what tests/test_alignment_gpu.py leans on: on
each of its ICP cases the float64 loop converges within the stated rounds, and at every round the nearest and the
second-nearest target of every query are at least 1e-4 apart (relative, squared distances), two orders above
float32's error in the difference form, so that a float32 search finds the same matches."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import alignment_reference as ar
from pytorch_mesh_renderer_amd import _native, mesh_renderer

points = mesh_renderer.points
TOL = 1e-12


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def _orthonormal(R, det, tol=1e-12):
    R = np.asarray(R, np.float64)
    assert np.isfinite(R).all()
    assert np.abs(R @ R.T - np.eye(3)).max() <= tol
    assert abs(np.linalg.det(R) - det) <= tol


def test_the_functions_are_exported():
    assert callable(points.corresponding_points_alignment) and callable(points.iterative_closest_point)
    assert points.SimilarityTransform._fields == ("R", "T", "s")
    assert points.ICPSolution._fields == ("converged", "rmse", "Xt", "RTs", "iterations")


@pytest.mark.parametrize("k", range(len(ar.ALIGNMENT_SHAPES)))
def test_torch_spelling_matches_the_restatement(k):
    case = ar.alignment_case(k)
    x, y = case["x"].astype(np.float64), case["y"].astype(np.float64)
    padded_x, padded_y = x.copy(), y.copy()
    for b, n in enumerate(case["lengths"]):
        padded_x[b, n:] = np.nan                                  # padding influences nothing, NaN included
        padded_y[b, n:] = np.nan
    for use_weights, use_lengths, scale, reflect in itertools.product((False, True), repeat=4):
        w = case["weights"].astype(np.float64) if use_weights else None
        n = case["lengths"] if use_lengths else None
        got = points.corresponding_points_alignment(
            _t(padded_x if use_lengths else x), _t(padded_y if use_lengths else y), None if w is None else _t(w),
            None if n is None else torch.as_tensor(n), estimate_scale=scale, allow_reflection=reflect)
        R, T, s, mse, sigma = ar.alignment_batch(x, y, w, n, scale, reflect)
        for b in range(len(x)):
            unique = sigma[b, 1] + sigma[b, 2] >= 0.05 * sigma[b, 0] and (sigma[b, 2] > 1e-9 * sigma[b, 0] or not reflect)
            if unique or sigma[b, 0] == 0:
                assert np.abs(got.R[b].numpy() - R[b]).max() <= TOL
                assert np.abs(got.T[b].numpy() - T[b]).max() <= TOL
            _orthonormal(got.R[b], np.linalg.det(R[b]))
            assert abs(float(got.s[b]) - s[b]) <= TOL * max(1.0, abs(s[b]))
            rows = slice(0, len(x[b]) if n is None else int(n[b]))
            if sigma[b, 0] > 0:
                mine = ar.residual_of(x[b][rows], y[b][rows], ar.Transform(got.R[b].numpy(), got.T[b].numpy(),
                                                                           float(got.s[b])),
                                      None if w is None else w[b][rows])
                assert abs(mine - mse[b]) <= TOL


def test_unbatched_inputs():
    case = ar.alignment_case(2)
    x, y, w = _t(case["x"][0]), _t(case["y"][0]), _t(case["weights"][0])
    got = points.corresponding_points_alignment(x, y, w, torch.tensor(40), estimate_scale=True)
    want, _, _ = ar.alignment(case["x"][0][:40], case["y"][0][:40], case["weights"][0][:40], True, False)
    assert got.R.shape == (3, 3) and got.T.shape == (3,) and got.s.shape == ()
    assert np.abs(got.R.numpy() - want.R).max() <= TOL and np.abs(got.T.numpy() - want.T).max() <= TOL
    assert abs(float(got.s) - want.s) <= TOL


def test_mirrored_cloud():
    x = ar.alignment_case(2)["x"][0].astype(np.float64)
    R = ar.rotation([2, -1, 1], 25.0).T
    mirror = R @ np.diag([1.0, 1.0, -1.0])
    y = 1.1 * x @ mirror + np.array([0.2, 0.1, -0.3])
    free = points.corresponding_points_alignment(_t(x), _t(y), estimate_scale=True, allow_reflection=True)
    assert np.abs(free.R.numpy() - mirror).max() <= 1e-12 and abs(float(free.s) - 1.1) <= 1e-12
    assert abs(np.linalg.det(free.R.numpy()) + 1) <= 1e-12
    proper = points.corresponding_points_alignment(_t(x), _t(y), estimate_scale=True)
    want, _, _ = ar.alignment(x, y, None, True, False)
    _orthonormal(proper.R.numpy(), 1.0)
    assert np.abs(proper.R.numpy() - want.R).max() <= TOL and abs(float(proper.s) - want.s) <= TOL


def degenerate_cases():
    """name -> (x [B,N,3], y, weights or None, lengths or None) float64 arrays: every degenerate input the interface
    defines."""
    rng = np.random.default_rng(77)
    x, y = rng.uniform(-1, 1, (1, 16, 3)), rng.uniform(-1, 1, (1, 16, 3))   # 16: the mean of equal points is exact
    line = np.linspace(-1, 1, 16)[None, :, None]
    return {
        "empty": (x, y, None, np.array([0])),
        "zero weights": (x, y, np.zeros((1, 16)), None),
        "coincident x": (np.repeat(x[:, :1], 16, axis=1), y, None, None),               # zero variance: s = 1, C = 0
        "coincident y": (x, np.repeat(y[:, :1], 16, axis=1), None, None),               # C = 0: R = I
        "collinear": (line * np.array([1.0, 2.0, -1.0]) + 0.3, line * np.array([0.5, 0.5, 2.0]) - 0.1, None, None),
        "one point": (x[:, :1], y[:, :1], None, None),
    }


@pytest.mark.parametrize("name", sorted(degenerate_cases()))
@pytest.mark.parametrize("reflect", [False, True])
def test_degenerate_inputs(name, reflect):
    x, y, w, n = degenerate_cases()[name]
    got = points.corresponding_points_alignment(_t(x), _t(y), None if w is None else _t(w),
                                                None if n is None else torch.as_tensor(n), estimate_scale=True,
                                                allow_reflection=reflect)
    R, T, s = got.R[0].numpy(), got.T[0].numpy(), float(got.s[0])
    if name in ("empty", "zero weights"):
        assert np.array_equal(R, np.eye(3)) and np.array_equal(T, np.zeros(3)) and s == 1.0
        return
    want, mse, _ = ar.alignment(x[0], y[0], None, True, reflect)
    _orthonormal(R, 1.0 if not reflect else round(np.linalg.det(R)))
    if name in ("coincident x", "coincident y", "one point"):
        assert np.abs(R - np.eye(3)).max() <= TOL
    if name in ("coincident x", "one point"):
        assert s == 1.0
    assert abs(ar.residual_of(x[0], y[0], ar.Transform(R, T, s)) - mse) <= TOL       # the minimum, whichever minimiser


def test_a_non_finite_coordinate_touches_only_its_image():
    case = ar.alignment_case(2)
    x, y = _t(case["x"]), _t(case["y"])
    lengths = torch.as_tensor(case["lengths"])
    clean = points.corresponding_points_alignment(x, y, lengths=lengths, estimate_scale=True)
    bad = x.clone()
    bad[1, 2, 1] = float("nan")
    got = points.corresponding_points_alignment(bad, y, lengths=lengths, estimate_scale=True)
    for mine, theirs in zip(got, clean):
        assert not torch.isfinite(mine[1]).any()
        assert torch.equal(mine[0], theirs[0]) and torch.equal(mine[2], theirs[2])


def test_argument_errors():
    x = torch.zeros(2, 5, 3)
    with pytest.raises(TypeError):
        points.corresponding_points_alignment(x.numpy(), x)
    with pytest.raises(TypeError):
        points.corresponding_points_alignment(x.long(), x.long())
    with pytest.raises(ValueError):
        points.corresponding_points_alignment(x, torch.zeros(2, 6, 3))
    with pytest.raises(ValueError):
        points.corresponding_points_alignment(x, x, weights=torch.zeros(2, 4))
    with pytest.raises(RuntimeError):
        points.corresponding_points_alignment(x, x.double())
    with pytest.raises(RuntimeError):
        points.corresponding_points_alignment(x, x, weights=torch.zeros(2, 5, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        points.corresponding_points_alignment(x, x, lengths=torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError):
        points.corresponding_points_alignment(x, x, lengths=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError):
        points.iterative_closest_point(x, torch.zeros(3, 5, 3))
    with pytest.raises(RuntimeError):
        points.iterative_closest_point(x, x.double())
    with pytest.raises(ValueError):
        points.iterative_closest_point(x, x, max_iterations=-1)
    with pytest.raises(ValueError):
        points.iterative_closest_point(x, x, check_every=1.5)
    with pytest.raises(ValueError):
        points.iterative_closest_point(x, x, max_correspondence_distance=-1.0)
    with pytest.raises(ValueError):
        points.iterative_closest_point(x, (x, torch.zeros(1, 3, dtype=torch.long)), y_lengths=torch.tensor([1, 1]))
    with pytest.raises(ValueError):
        points.iterative_closest_point(x, x, init_transform=(torch.eye(3), torch.zeros(3), torch.ones(1)))
    with pytest.raises(RuntimeError):
        points.iterative_closest_point(x, (x, torch.zeros(1, 3)))


def test_gradcheck_of_the_torch_spelling():
    case = ar.alignment_case(2)
    x = _t(case["x"][:2, :12]).requires_grad_(True)
    y = _t(case["y"][:2, :12]).requires_grad_(True)
    w = (_t(case["weights"][:2, :12]) + 0.1).requires_grad_(True)

    def f(x, y, w):
        out = points.corresponding_points_alignment(x, y, w, estimate_scale=True)
        return out.R, out.T, out.s
    assert torch.autograd.gradcheck(f, (x, y, w), eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("case", ar.ICP_CLOUD_CASES)
def test_icp_cases_converge_with_a_gap(case):
    M, N, degrees, scale, seed, rounds = case
    x, y, R = ar.icp_cloud_case(M, N, degrees, scale, seed)
    want = ar.icp(x, y, max_iterations=20, estimate_scale=scale != 1.0)
    print(case, want.iterations, want.rmse, min(want.gaps))
    assert want.converged and want.iterations <= rounds
    assert np.array_equal(want.matches, np.arange(N))
    assert min(want.gaps) >= 1e-4
    assert want.rmse <= 1e-7 and ar.angle_between(want.R, R) <= 1e-5
    # the torch spelling of the loop, in float64: the same rounds, the same result
    got = points.iterative_closest_point(_t(x), _t(y), max_iterations=20, estimate_scale=scale != 1.0, check_every=1)
    assert bool(got.converged) and int(got.iterations) == want.iterations
    assert np.abs(got.RTs.R.numpy() - want.R).max() <= 1e-9 and abs(float(got.rmse) - want.rmse) <= 1e-9
    assert np.abs(got.Xt.numpy() - want.Xt).max() <= 1e-9


def test_icp_torch_batch_equals_single_calls_and_freezes():
    cases = [ar.icp_cloud_case(*c[:5]) for c in ar.ICP_CLOUD_CASES[:3]]
    x = torch.stack([_t(c[0]) for c in cases] + [torch.full((150, 3), float("nan"), dtype=torch.float64)])
    y = torch.stack([_t(c[1]) for c in cases] + [_t(cases[0][1])])
    lengths = torch.tensor([150, 150, 150, 0])
    batch = points.iterative_closest_point(x, y, x_lengths=lengths, max_iterations=20, estimate_scale=True, check_every=0)
    assert bool(batch.converged.all()) and int(batch.iterations[3]) == 1 and float(batch.rmse[3]) == 0.0
    assert torch.equal(batch.RTs.R[3], torch.eye(3, dtype=torch.float64)) and not batch.Xt[3].any()
    for b in range(3):
        one = points.iterative_closest_point(x[b], y[b], max_iterations=20, estimate_scale=True, check_every=1)
        assert int(one.iterations) == int(batch.iterations[b])
        assert torch.allclose(one.RTs.R, batch.RTs.R[b], atol=1e-12, rtol=0)
        assert abs(float(one.rmse) - float(batch.rmse[b])) <= 1e-12


def test_icp_on_the_cube_mesh_in_torch():
    scan, R, T, scale = ar.cube_scan(300, 8.0)
    v, t = ar.cube_mesh()
    want = ar.icp(scan, closest_point=ar.mesh_closest_point(v, t), max_iterations=30, estimate_scale=True,
                  relative_rmse_thr=0.0)
    got = points.iterative_closest_point(_t(scan), (_t(v), torch.as_tensor(t)), max_iterations=30, estimate_scale=True,
                                         relative_rmse_thr=0.0, check_every=0)
    print(ar.angle_between(want.R, R), ar.angle_between(got.RTs.R.numpy(), R))
    assert ar.angle_between(want.R, R) <= 0.05
    assert ar.angle_between(got.RTs.R.numpy(), R) <= 2 * ar.angle_between(want.R, R) + 1e-4


def test_native_validation_without_a_gpu():
    L = _native.lib()
    assert L.mr_align_workspace_bytes(1, 1) == 256
    assert L.mr_align_workspace_bytes(64, 300) == 64 * 144
    assert L.mr_align_workspace_bytes(1, 100000) == (98 * 144 + 255) // 256 * 256
    bad = [(0, 5), (65536, 5), (1, 0), (1, (1 << 28) + 1), (65535, 1 << 21)]
    one = ctypes.c_void_p(256)   # never dereferenced: every call below is refused before a device is touched
    for B, N in bad:
        assert L.mr_align_workspace_bytes(B, N) == 0
        assert L.mr_align_solve(one, one, None, 0, None, None, 0.0, None, B, N, N, 0, 0, 0.0, one, one, one, None, None,
                                None, None, one, 1 << 30, None) == _native.MR_EINVAL
        assert L.mr_align_apply(one, None, one, one, one, B, N, one, None) == _native.MR_EINVAL
        assert L.mr_align_closest_points(one, one, one, one, B, N, 3, 1, one, None) == _native.MR_EINVAL
    solve = lambda *a: L.mr_align_solve(*a)
    ok_tail = (one, one, one, None, None, None, None, one, 1 << 30, None)
    assert solve(None, one, None, 0, None, None, 0.0, None, 1, 5, 5, 0, 0, 0.0, *ok_tail) == _native.MR_EINVAL
    assert solve(one, one, None, 1, None, None, 0.0, None, 1, 5, 9, 0, 0, 0.0, *ok_tail) == _native.MR_EINVAL   # no idx
    assert solve(one, one, None, 0, None, None, 0.0, None, 1, 5, 9, 0, 0, 0.0, *ok_tail) == _native.MR_EINVAL   # M != N
    assert solve(one, one, None, 0, None, None, 0.0, None, 1, 5, 5, 0, 0, 0.0, one, one, one, None, one, None, None, one,
                 1 << 30, None) == _native.MR_EINVAL                                  # half of ICP's bookkeeping
    assert solve(one, one, None, 0, None, None, 0.0, None, 1, 5, 5, 0, 0, 0.0, one, one, one, None, None, None, None, one,
                 16, None) == _native.MR_EWORKSPACE
    assert L.mr_align_icp_init(None, None, None, 0, one, one, one, one, one, one, one, None) == _native.MR_EINVAL
    assert L.mr_align_icp_init(one, None, None, 1, one, one, one, one, one, one, one, None) == _native.MR_EINVAL
    assert L.mr_align_closest_points(one, one, one, one, 1, 5, 0, 1, one, None) == _native.MR_EINVAL
    x = torch.zeros(1, 5, 3)
    with pytest.raises(RuntimeError):
        _native.align_solve(x, x)                                  # host tensors never reach the library
    with pytest.raises(RuntimeError):
        _native.align_solve(x.double(), x.double())
    with pytest.raises(ValueError):
        _native.align_solve(x, torch.zeros(1, 6, 3))
    with pytest.raises(ValueError):
        _native.icp(x)
