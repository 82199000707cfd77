"""mesh_renderer.points.corresponding_points_alignment and iterative_closest_point on the MI355X (csrc/align.hip)
against the numpy float64 restatement (tests/alignment_reference.py) on the same float32 inputs.

Alignment.  The kernels compute in float64 and round once, so where the minimiser is unique and well conditioned
(sigma_2 + sigma_3 >= 0.05 sigma_1 of the covariance; with allow_reflection also sigma_3 > 0, since a flat cloud's
mirror image fits equally well) |R - R64| <= 2^-23, and T and s are within one float32 ulp of their magnitude
(floor 2^-23).  Elsewhere the residual of the returned transform is compared with the minimum: the gradient of the
residual in R is at most 2 (s^2 var x + var y), each entry of R is rounded by at most 2^-24, hence RESIDUAL_UNITS x
2^-24 x (s^2 var x + var y) with RESIDUAL_UNITS = 2 x 9 = 18.

ICP.  tests/test_alignment_host.py establishes that on the planted cases the float64 loop converges and that at every
round every query's nearest and second-nearest target are >= 1e-4 apart, so the float32 search finds the same matches
and the loops may be compared round for round.  The mesh target's restatement takes its closest points from
tests/point_mesh_reference.py (float64, brute force over the triangles)."""
import itertools

import numpy as np
import pytest
import torch

import alignment_reference as ar
from pytorch_mesh_renderer_amd import _native, mesh_renderer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
points = mesh_renderer.points
EPS = 2.0 ** -23
RESIDUAL_UNITS = 18


def _d(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).to(DEV)


def _ulp(v):
    return np.maximum(np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64), EPS)


def _variance(a, w):
    a = a.astype(np.float64)
    mean = np.average(a, axis=0, weights=w)
    return float(np.average(((a - mean) ** 2).sum(-1), weights=w))


def _check_alignment(got, x, y, w, n, scale, reflect, what, compare_T=True, residual=True):
    """got: the device result for the float32 arrays x, y [B,N,3] (w [B,N], n [B] or None).  residual: also hold the
    residual of the returned transform to the minimum (clouds near the origin only: far away the rounding of R and T
    moves every point by an ulp of its coordinates).  -> the worst |R - R64| over the images that assert it."""
    R64, T64, s64, mse, sigma = ar.alignment_batch(x, y, w, n, scale, reflect)
    R, T, s = (t.cpu().numpy().astype(np.float64) for t in (got.R, got.T, got.s))
    assert got.R.dtype == torch.float32 and got.R.is_cuda and R.shape == R64.shape and T.shape == T64.shape
    worst = 0.0
    for b in range(len(x)):
        where = "%s image %d" % (what, b)
        unique = sigma[b, 1] + sigma[b, 2] >= 0.05 * sigma[b, 0] and (sigma[b, 2] > 1e-6 * sigma[b, 0] or not reflect)
        assert np.isfinite(R[b]).all() and np.abs(R[b] @ R[b].T - np.eye(3)).max() <= 4 * EPS, where
        if reflect and not unique:   # a flat cloud and its mirror image fit equally well: either determinant
            assert abs(abs(np.linalg.det(R[b])) - 1) <= 4 * EPS, where
        else:
            assert abs(np.linalg.det(R[b]) - np.linalg.det(R64[b])) <= 4 * EPS, where
        if unique or sigma[b, 0] == 0:
            worst = max(worst, np.abs(R[b] - R64[b]).max())
            assert np.abs(R[b] - R64[b]).max() <= EPS, (where, np.abs(R[b] - R64[b]).max())
            assert abs(s[b] - s64[b]) <= _ulp(s64[b]), (where, s[b], s64[b])
            if compare_T:
                assert (np.abs(T[b] - T64[b]) <= _ulp(T64[b])).all(), (where, T[b], T64[b])
        if residual and sigma[b, 0] > 0:
            rows = slice(0, len(x[b]) if n is None else int(np.clip(n[b], 0, len(x[b]))))
            wb = None if w is None else w[b][rows]
            mine = ar.residual_of(x[b][rows], y[b][rows], ar.Transform(R[b], T[b], s[b]), wb)
            bound = RESIDUAL_UNITS * 2.0 ** -24 * (s64[b] ** 2 * _variance(x[b][rows], wb) + _variance(y[b][rows], wb))
            assert abs(mine - mse[b]) <= bound + 1e-13, (where, mine, mse[b], bound)
    return worst


@pytest.mark.parametrize("k", range(len(ar.ALIGNMENT_SHAPES)))
def test_alignment_matches_the_restatement(k):
    case = ar.alignment_case(k)
    x, y = case["x"], case["y"]
    padded_x, padded_y = x.copy(), y.copy()
    for b, n in enumerate(case["lengths"]):
        padded_x[b, n:] = np.nan
        padded_y[b, n:] = np.nan
    worst = 0.0
    for use_weights, use_lengths, scale, reflect in itertools.product((False, True), repeat=4):
        w = case["weights"] if use_weights else None
        n = case["lengths"] if use_lengths else None
        got = points.corresponding_points_alignment(
            _d(padded_x if use_lengths else x), _d(padded_y if use_lengths else y), None if w is None else _d(w),
            None if n is None else _d(n, torch.int32), estimate_scale=scale, allow_reflection=reflect)
        worst = max(worst, _check_alignment(got, x, y, w, n, scale, reflect,
                                            "shape %d %s" % (k, (use_weights, use_lengths, scale, reflect))))
    print("shape", ar.ALIGNMENT_SHAPES[k], "worst |R - R64| = %.3g (bound %.3g)" % (worst, EPS))


def test_unbatched_inputs_and_native_rmse():
    case = ar.alignment_case(2)
    got = points.corresponding_points_alignment(_d(case["x"][0]), _d(case["y"][0]), _d(case["weights"][0]),
                                                torch.tensor(40, device=DEV), estimate_scale=True)
    assert got.R.shape == (3, 3) and got.T.shape == (3,) and got.s.shape == ()
    want, mse, _ = ar.alignment(case["x"][0][:40], case["y"][0][:40], case["weights"][0][:40], True, False)
    assert np.abs(got.R.cpu().numpy() - want.R).max() <= EPS
    lengths = torch.tensor([40, 63, 0], device=DEV, dtype=torch.int32)
    R, T, s, rmse = _native.align_solve(_d(case["x"]), _d(case["y"]), _d(case["weights"]), lengths, estimate_scale=True)
    assert abs(float(rmse[0]) - np.sqrt(mse)) <= 2 * EPS * np.sqrt(mse) and float(rmse[2]) == 0.0
    assert torch.equal(R[0], got.R) and torch.equal(T[0], got.T) and torch.equal(s[0], got.s)
    assert torch.equal(R[2], torch.eye(3, device=DEV)) and not T[2].any() and float(s[2]) == 1.0     # W = 0
    xt = _native.align_apply(_d(case["x"]), R, T, s, lengths).cpu().numpy()
    assert not xt[0, 40:].any() and not xt[2].any()
    want_xt = want.s * case["x"][0][:40].astype(np.float64) @ want.R + want.T
    # |xt| < 4: five float32 roundings of at most half an ulp there (2.4e-7 each), and R, T, s rounded once
    assert np.abs(xt[0, :40] - want_xt).max() <= 3e-6


@pytest.mark.parametrize("k", [2, 3, 4])
def test_translated_clouds_give_the_same_rotation_and_scale(k):
    """Both clouds on a grid of 2^-10, so that adding (1000, -2000, 500) is exact in float32: the far clouds hold the
    same shapes, and the moments about a pivot lose nothing to |x|^2 ~ 5e6."""
    case = ar.alignment_case(k)
    offset = np.array([1000.0, -2000.0, 500.0], np.float32)
    x, y = np.round(case["x"] * 1024) / 1024, np.round(case["y"] * 1024) / 1024
    far_x, far_y = (x + offset).astype(np.float32), (y + offset).astype(np.float32)
    assert np.array_equal(far_x.astype(np.float64) - offset, x) and np.array_equal(far_y.astype(np.float64) - offset, y)
    for use_weights, scale in itertools.product((False, True), repeat=2):
        w = case["weights"] if use_weights else None
        near = points.corresponding_points_alignment(_d(x), _d(y), None if w is None else _d(w), estimate_scale=scale)
        far = points.corresponding_points_alignment(_d(far_x), _d(far_y), None if w is None else _d(w),
                                                    estimate_scale=scale)
        _check_alignment(near, x.astype(np.float32), y.astype(np.float32), w, None, scale, False, "near %d" % k)
        _check_alignment(far, x.astype(np.float32), y.astype(np.float32), w, None, scale, False, "far %d" % k,
                         compare_T=False, residual=False)
        _check_alignment(far, far_x, far_y, w, None, scale, False, "far against far %d" % k, residual=False)


def _degenerate():
    rng = np.random.default_rng(77)
    x, y = rng.uniform(-1, 1, (1, 16, 3)).astype(np.float32), rng.uniform(-1, 1, (1, 16, 3)).astype(np.float32)
    line = (np.arange(16, dtype=np.float32) / 8 - 1)[None, :, None]               # exact in float32
    return {
        "empty": (x, y, None, np.array([0], np.int32)),
        "zero weights": (x, y, np.zeros((1, 16), np.float32), None),
        "coincident x": (np.repeat(x[:, :1], 16, axis=1), y, None, None),
        "coincident y": (x, np.repeat(y[:, :1], 16, axis=1), None, None),
        "coincident both": (np.repeat(x[:, :1], 16, axis=1), np.repeat(y[:, :1], 16, axis=1), None, None),
        "collinear": (line * np.array([1.0, 2.0, -1.0], np.float32) + np.float32(0.25),
                      line * np.array([0.5, 0.5, 2.0], np.float32) - np.float32(0.125), None, None),
        "one point": (x[:, :1], y[:, :1], None, None),
    }


@pytest.mark.parametrize("name", sorted(_degenerate()))
@pytest.mark.parametrize("reflect", [False, True])
def test_degenerate_inputs(name, reflect):
    x, y, w, n = _degenerate()[name]
    got = points.corresponding_points_alignment(_d(x), _d(y), None if w is None else _d(w),
                                                None if n is None else _d(n, torch.int32), estimate_scale=True,
                                                allow_reflection=reflect)
    R, T, s = got.R[0].cpu().numpy().astype(np.float64), got.T[0].cpu().numpy().astype(np.float64), float(got.s[0])
    if name in ("empty", "zero weights"):
        assert np.array_equal(R, np.eye(3)) and np.array_equal(T, np.zeros(3)) and s == 1.0
        return
    assert np.isfinite(R).all() and np.abs(R @ R.T - np.eye(3)).max() <= 4 * EPS
    det = np.linalg.det(R)
    assert abs(det - 1) <= 4 * EPS or (reflect and abs(det + 1) <= 4 * EPS)
    if name.startswith("coincident") or name == "one point":
        assert np.array_equal(R, np.eye(3))
    if name in ("coincident x", "coincident both", "one point"):
        assert s == 1.0
    _check_alignment(got, x, y, w, n, True, reflect, name)                         # the residual is the minimum


def test_a_nan_leaves_the_other_images_bit_identical():
    case = ar.alignment_case(2)
    x, y, w = _d(case["x"]), _d(case["y"]), _d(case["weights"])
    n = _d(case["lengths"], torch.int32)
    clean = _native.align_solve(x, y, w, n, estimate_scale=True)
    for tensor, value in ((x, float("nan")), (y, float("inf")), (w, float("nan"))):
        bad = tensor.clone()
        bad[1, 2] = value
        args = [bad if t is tensor else t for t in (x, y, w)]
        got = _native.align_solve(*args, n, estimate_scale=True)
        for mine, theirs in zip(got, clean):
            assert not torch.isfinite(mine[1]).any()
            assert torch.equal(mine[0], theirs[0]) and torch.equal(mine[2], theirs[2])
    beyond = x.clone()
    beyond[1, int(case["lengths"][1]):] = float("nan")               # in the padding: nothing happens
    for mine, theirs in zip(_native.align_solve(beyond, y, w, n, estimate_scale=True), clean):
        assert torch.equal(mine, theirs)


# ---- ICP ------------------------------------------------------------------------------------------------------------

_icp_truth = {}


def _icp_case(k):
    """-> (x, y float32 arrays, planted R, the restatement's run), computed once."""
    if k not in _icp_truth:
        M, N, degrees, scale, seed, _ = ar.ICP_CLOUD_CASES[k]
        x, y, R = ar.icp_cloud_case(M, N, degrees, scale, seed)
        _icp_truth[k] = (x, y, R, ar.icp(x, y, max_iterations=20, estimate_scale=scale != 1.0))
    return _icp_truth[k]


@pytest.mark.parametrize("k", range(len(ar.ICP_CLOUD_CASES)))
def test_icp_on_a_cloud(k):
    x, y, R, want = _icp_case(k)
    scale = ar.ICP_CLOUD_CASES[k][3]
    got = points.iterative_closest_point(_d(x), _d(y), max_iterations=20, estimate_scale=scale != 1.0)
    angle = ar.angle_between(got.RTs.R.cpu().numpy(), R)
    print("case %d: iterations %d (restatement %d), rmse %.3g (%.3g), angle error %.3g deg, s %.8f" % (
        k, int(got.iterations), want.iterations, float(got.rmse), want.rmse, angle, float(got.RTs.s)))
    assert got.converged.dtype == torch.bool and got.iterations.dtype == torch.int32 and got.Xt.shape == x.shape
    assert bool(got.converged)
    _, idx = points.nearest_points(got.Xt, _d(y))
    assert np.array_equal(idx.cpu().numpy(), np.arange(len(x)))
    assert abs(int(got.iterations) - want.iterations) <= 1
    assert float(got.rmse) <= 2 * want.rmse + 1e-7
    assert angle <= 1e-4
    assert abs(float(got.RTs.s) - scale) <= 1e-5
    assert torch.equal(got.Xt, _native.align_apply(_d(x)[None], got.RTs.R[None], got.RTs.T[None], got.RTs.s[None])[0])


def _batch():
    """The four cloud cases padded into one batch, plus an image without queries and one without targets."""
    cases = [_icp_case(k) for k in range(4)]
    x = torch.full((6, 257, 3), float("nan"))
    y = torch.full((6, 1000, 3), float("nan"))
    for b, (cx, cy, _, _) in enumerate(cases):
        x[b, :len(cx)], y[b, :len(cy)] = torch.as_tensor(cx), torch.as_tensor(cy)
    x[4], y[4], x[5], y[5] = x[0], y[0], x[1], y[1]
    x_lengths = torch.tensor([len(c[0]) for c in cases] + [0, 150], dtype=torch.int32)
    y_lengths = torch.tensor([len(c[1]) for c in cases] + [400, 0], dtype=torch.int32)
    return cases, x.to(DEV), y.to(DEV), x_lengths.to(DEV), y_lengths.to(DEV)


def _same(a, b):
    return all(torch.equal(p, q) for p, q in ((a.RTs.R, b.RTs.R), (a.RTs.T, b.RTs.T), (a.RTs.s, b.RTs.s),
                                              (a.rmse, b.rmse), (a.iterations, b.iterations), (a.converged, b.converged)))


def test_icp_batch_equals_the_single_calls_bit_for_bit():
    cases, x, y, x_lengths, y_lengths = _batch()
    batch = points.iterative_closest_point(x, y, x_lengths, y_lengths, max_iterations=20, estimate_scale=True)
    print("iterations", batch.iterations.tolist())
    assert bool(batch.converged.all())
    for b, (cx, cy, _, _) in enumerate(cases):
        one = points.iterative_closest_point(_d(cx), _d(cy), max_iterations=20, estimate_scale=True)
        assert torch.equal(one.RTs.R, batch.RTs.R[b]) and torch.equal(one.RTs.T, batch.RTs.T[b]), b
        assert torch.equal(one.RTs.s, batch.RTs.s[b]) and torch.equal(one.rmse, batch.rmse[b]), b
        assert torch.equal(one.iterations, batch.iterations[b]) and bool(one.converged), b
        assert torch.equal(one.Xt, batch.Xt[b, :len(cx)]) and not batch.Xt[b, len(cx):].any()
    for b in (4, 5):                                                  # no query / no target: done at once, untouched
        assert int(batch.iterations[b]) == 1 and float(batch.rmse[b]) == 0.0
        assert torch.equal(batch.RTs.R[b], torch.eye(3, device=DEV)) and not batch.RTs.T[b].any()
        assert float(batch.RTs.s[b]) == 1.0
    assert not batch.Xt[4].any() and torch.equal(batch.Xt[5, :150], x[5, :150])
    # the host's early stop changes nothing: never reading back, and reading back after every round
    never = points.iterative_closest_point(x, y, x_lengths, y_lengths, max_iterations=20, estimate_scale=True,
                                           check_every=0)
    always = points.iterative_closest_point(x, y, x_lengths, y_lengths, max_iterations=20, estimate_scale=True,
                                            check_every=1)
    assert _same(never, always) and _same(never, batch)
    assert torch.equal(never.Xt, always.Xt)


def test_icp_init_transform_and_unconverged():
    x, y, R, want = _icp_case(2)
    short = points.iterative_closest_point(_d(x), _d(y), max_iterations=2)
    assert not bool(short.converged) and int(short.iterations) == 2
    resumed = points.iterative_closest_point(_d(x), _d(y), init_transform=short.RTs, max_iterations=20)
    assert bool(resumed.converged) and ar.angle_between(resumed.RTs.R.cpu().numpy(), R) <= 1e-4
    none = points.iterative_closest_point(_d(x), _d(y), init_transform=short.RTs, max_iterations=0)
    assert torch.equal(none.RTs.R, short.RTs.R) and int(none.iterations) == 0 and torch.equal(none.Xt, short.Xt)


def test_icp_cut_off_drops_far_outliers():
    x, y, R, want = _icp_case(1)
    rng = np.random.default_rng(5)
    far = (rng.uniform(-1, 1, (30, 3)) + np.array([6.0, -7.0, 8.0])).astype(np.float32)
    dirty = np.concatenate([x, far])
    clean = points.iterative_closest_point(_d(x), _d(y), max_iterations=20, estimate_scale=True,
                                           max_correspondence_distance=0.6)
    got = points.iterative_closest_point(_d(dirty), _d(y), max_iterations=20, estimate_scale=True,
                                         max_correspondence_distance=0.6)
    assert bool(got.converged) and bool(clean.converged)
    assert ar.angle_between(clean.RTs.R.cpu().numpy(), R) <= 1e-4
    for mine, theirs in zip(got.RTs, clean.RTs):
        assert float((mine - theirs).abs().max()) <= 1e-6
    assert abs(float(got.rmse) - float(clean.rmse)) <= 1e-6 and int(got.iterations) == int(clean.iterations)
    # their weight is 0: without the cut-off they drag the transform away
    dragged = points.iterative_closest_point(_d(dirty), _d(y), max_iterations=20, estimate_scale=True)
    assert ar.angle_between(dragged.RTs.R.cpu().numpy(), R) > 1.0
    nothing = points.iterative_closest_point(_d(far), _d(y), max_iterations=20, max_correspondence_distance=0.6)
    assert bool(nothing.converged) and int(nothing.iterations) == 1 and float(nothing.rmse) == 0.0
    assert torch.equal(nothing.RTs.R, torch.eye(3, device=DEV)) and torch.equal(nothing.Xt, _d(far))


def test_icp_on_a_mesh_target():
    scan, R, T, scale = ar.cube_scan(300, 8.0)
    v, t = ar.cube_mesh()
    want = ar.icp(scan, closest_point=ar.mesh_closest_point(v, t), max_iterations=30, estimate_scale=True,
                  relative_rmse_thr=-1.0)
    got = points.iterative_closest_point(_d(scan), (_d(v), torch.as_tensor(t, device=DEV)), max_iterations=30,
                                         estimate_scale=True, relative_rmse_thr=-1.0, check_every=0)
    mine, theirs = ar.angle_between(got.RTs.R.cpu().numpy(), R), ar.angle_between(want.R, R)
    print("cube, 300 points, 8 deg, 30 rounds: angle error %.3g deg (restatement %.3g), s %.7f" % (
        mine, theirs, float(got.RTs.s)))
    assert int(got.iterations) == want.iterations == 30
    assert mine <= 2 * theirs + 1e-4
    batch = points.iterative_closest_point(_d(np.stack([scan, scan[::-1]])), (_d(np.stack([v, v])),
                                           torch.as_tensor(t, device=DEV)), x_lengths=torch.tensor([300, 120], device=DEV),
                                           max_iterations=30, estimate_scale=True, relative_rmse_thr=-1.0, check_every=0)
    assert torch.equal(batch.RTs.R[0], got.RTs.R) and torch.equal(batch.rmse[0], got.rmse)
    assert not batch.Xt[1, 120:].any()


def _run_everything():
    cases, x, y, x_lengths, y_lengths = _batch()
    case = ar.alignment_case(3)
    solved = _native.align_solve(_d(case["x"]), _d(case["y"]), _d(case["weights"]), estimate_scale=True)
    out = points.iterative_closest_point(x, y, x_lengths, y_lengths, max_iterations=20, estimate_scale=True)
    return list(solved) + [out.RTs.R, out.RTs.T, out.RTs.s, out.rmse, out.iterations, out.Xt]


def test_two_runs_are_bit_identical_in_either_deterministic_mode():
    before = _native.set_deterministic(False)
    try:
        runs = []
        for mode in (False, False, True, True):
            _native.set_deterministic(mode)
            runs.append(_run_everything())
    finally:
        _native.set_deterministic(before)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def test_captured_loop_replays_to_the_eager_result():
    x0, y0, _, _ = _icp_case(0)
    x1, y1, _, _ = _icp_case(2)
    run = lambda x, y: points.iterative_closest_point(x, y, max_iterations=8, estimate_scale=True, check_every=0)
    static_x, static_y = _d(x0)[None].clone(), _d(y0)[None].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static_x, static_y)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(static_x, static_y)
    static_x.copy_(_d(x1)[None])
    static_y.copy_(_d(y1)[None])
    graph.replay()
    eager = run(_d(x1)[None], _d(y1)[None])
    assert _same(captured, eager) and torch.equal(captured.Xt, eager.Xt)
    assert not torch.equal(captured.RTs.R, run(_d(x0)[None], _d(y0)[None]).RTs.R)
