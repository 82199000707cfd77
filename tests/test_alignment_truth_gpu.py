"""csrc/align.hip on the MI355X against the numpy float64 truth (tests/alignment_reference.py) in every regime of its
solve, with the cases and the check of tests/alignment_regimes.py (tests/test_alignment_truth_host.py establishes on
the CPU that every case sits in the regime it states).  The bounds are those tests/test_alignment_gpu.py derives:
where R is unique |R - R64| <= 2^-23 = 1.19e-7, s and T within one float32 ulp (floor 2^-23), orthonormality and
determinant within 4 x 2^-23; elsewhere the residual within 18 x 2^-24 x (s^2 var x + var y) of the minimum.

  regimes     all 48 signed permutations (the Jacobi rotates nothing), rotations by 90, 120, 179.999, 180 and 1e-5
              degrees and the identity, a mirror with and without allow_reflection, equal and two equal singular values
              (a cube's corners; mirrored, g = 0: residual only), exactly planar clouds, slabs whose third singular
              value runs from 1.9e-5 to 2.3e-14 of the first across the rank tolerance of 1e-13 -- as one padded batch
              under the four combinations of estimate_scale and allow_reflection, and some as single calls that must
              equal the batch bit for bit.
  scaling     x by 2^a, y by 2^b, weights by 2^+-100: every operation before the final rounding scales by a whole power
              of two, so R is bit-identical, s bit-identical times 2^(b-a), T bit-identical times 2^b.
  sentinels   rows at +-1e4, +-1e6, +-3e38 that are not counted -- weight 0, idx = -1, sqdist above the cut-off, a NaN
              sqdist -- at row 0, at row 1024 (the first of chunk 1), filling chunk 2: the truth of the kept rows.
  gather      _native.align_solve through an idx plane with repeats, -1 and entries >= M, with and without weights,
              lengths and the cut-off; and the plane only marking rows.
  shapes      N = 8193 and 20000 (nine and twenty chunks: the solve's interleaved sum takes a second and a third
              step), B = 2 with a 300-row image that must equal its single call bit for bit; _native.align_apply at
              N = 2^20 + 300, past its grid of 4096 workgroups.

WORST MEASURED |R - R64| on the MI355X (2026-10-21), bound 1.19e-7, per family: signed permutations 1.42e-8 (4.4e-16
with reflection allowed), general rotations 2.96e-8, mirror 2.93e-8, equal singular values 2.11e-8, planar 2.06e-8,
slabs 2.68e-8 (nothing moves across the rank tolerance: 2^-21 and 2^-22 mirrored both within 2.7e-8); sentinels 2.73e-8,
the same figure for 1e4, 1e6 and 3e38 and for each of the four ways; gather 2.87e-8 either way; N = 8193 2.69e-8,
N = 20000 2.78e-8; the apply 2.83e-7 of its 3e-6.  The scaled calls were bit-identical, and the ICP run with the
outliers first equalled the clean run bit for bit.  Before the moments took a chunk's own first counted row as their
reference point (they took row 0 of x and of the target, counted or not) the sentinel at row 0 gave 6.7e-8, 1.2e-3 and
1.35 on the base cloud, 3.2e-8, 4.7e-4 and 1.29 on the 2100-row cloud for 1e4, 1e6 and 3e38, in each of the four
ways, and the ICP run an rmse of 1.6e-3 against 2.6e-8; every other test here passed."""
import itertools

import numpy as np
import pytest
import torch

import alignment_reference as ar
import alignment_regimes as regimes
from pytorch_mesh_renderer_amd import _native, mesh_renderer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
points = mesh_renderer.points
EPS = regimes.EPS


def _d(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).to(DEV)


def _n(t):
    return t.cpu().numpy().astype(np.float64)


def _held(R, T, s, x, y, w, scale, reflect, expects_unique, what, known=None):
    """Prints the measured |R - R64| (before anything is asserted), then regimes.check at the float32 bounds."""
    known = known or regimes.truth(x, y, w, scale, reflect)
    R, T, s = _n(R), _n(T), float(s)
    print("%s: |R - R64| = %.3g%s" % (what, np.abs(R - known[0].R).max(), "" if known[5] else " (not unique)"))
    return regimes.check(R, T, s, x, y, w, scale, reflect, expects_unique, what, known=known)


# ---- the regimes --------------------------------------------------------------------------------------------------

_batch_results = {}


def _regime_batch(scale, reflect):
    if (scale, reflect) not in _batch_results:
        x, y, w, n = regimes.padded_batch(regimes.regime_cases())
        _batch_results[scale, reflect] = points.corresponding_points_alignment(
            _d(x), _d(y), _d(w), _d(n, torch.int32), estimate_scale=scale, allow_reflection=reflect)
    return _batch_results[scale, reflect]


@pytest.mark.parametrize("scale,reflect", list(itertools.product((False, True), repeat=2)))
def test_every_regime_in_one_batch(scale, reflect):
    got = _regime_batch(scale, reflect)
    worst = {}
    for b, (name, x, y, w, expects, family) in enumerate(regimes.regime_cases()):
        err = _held(got.R[b], got.T[b], got.s[b], x, y, w, scale, reflect, expects[reflect], name)
        if err is not None:
            worst[family] = max(worst.get(family, 0.0), err)
    print("WORST", (scale, reflect), " ".join("%s %.3g" % item for item in worst.items()))


SINGLE = ("perm 120 +++", "perm 012 ++-", "perm 201 -+-", "rotation 180", "rotation 1e-05", "mirror", "cube",
          "cube mirrored", "planar mirrored in the plane", "slab 2^-21 mirrored", "slab 2^-22 mirrored")


@pytest.mark.parametrize("reflect", [False, True])
def test_single_calls_equal_the_batch_bit_for_bit(reflect):
    cases = regimes.regime_cases()
    names = [c[0] for c in cases]
    batch = _regime_batch(True, reflect)
    for name in SINGLE:
        b = names.index(name)
        _, x, y, w, expects, _ = cases[b]
        one = points.corresponding_points_alignment(_d(x), _d(y), estimate_scale=True, allow_reflection=reflect)
        _held(one.R, one.T, one.s, x, y, w, True, reflect, expects[reflect], name + " alone")
        assert torch.equal(one.R, batch.R[b]) and torch.equal(one.T, batch.T[b]) and torch.equal(one.s, batch.s[b]), name


@pytest.mark.parametrize("reflect", [False, True])
def test_scaling_by_powers_of_two_is_exact(reflect):
    x, y, w, n = regimes.padded_batch(regimes.regime_cases())
    w = w * np.where(np.arange(w.shape[1]) % 3 == 0, np.float32(0.75), np.float32(0.5))       # stays on a 2^-10 grid
    run = lambda x, y, w, scale=True: points.corresponding_points_alignment(
        _d(x), _d(y), _d(w), _d(n, torch.int32), estimate_scale=scale, allow_reflection=reflect)
    plain, rigid = run(x, y, w), run(x, y, w, False)
    for a, b in ((40, 40), (-40, -40), (0, 20)):
        fx, fy = np.float32(2.0 ** a), np.float32(2.0 ** b)
        got = run(x * fx, y * fy, w)
        assert torch.equal(got.R, plain.R), (a, b, float((got.R - plain.R).abs().max()))
        assert torch.equal(got.s, plain.s * float(2.0 ** (b - a))), (a, b)
        assert torch.equal(got.T, plain.T * float(fy)), (a, b)
        assert torch.equal(run(x * fx, y * fy, w, False).R, rigid.R), (a, b)
    for c in (100, -100):
        got = run(x, y, w * np.float32(2.0 ** c))
        assert torch.equal(got.R, plain.R) and torch.equal(got.s, plain.s) and torch.equal(got.T, plain.T), c


# ---- rows that must influence nothing -------------------------------------------------------------------------------

def _without(way, x, y, kept):
    """The result with the rows outside `kept` taken out of the count in the given way."""
    rows = np.arange(len(x))
    if way == "weight 0":
        return points.corresponding_points_alignment(_d(x), _d(y), _d(kept), estimate_scale=True)
    if way == "idx -1":
        extra = dict(idx=_d(np.where(kept, rows, -1)[None], torch.int32))
    elif way == "sqdist above":
        extra = dict(sqdist=_d(np.where(kept, 0.5, 2.0)[None]), max_sqdist=1.0)
    else:
        extra = dict(sqdist=_d(np.where(kept, 0.5, np.nan)[None]), max_sqdist=1.0)
    R, T, s, _ = _native.align_solve(_d(x)[None], _d(y)[None], estimate_scale=True, **extra)
    return points.SimilarityTransform(R[0], T[0], s[0])


@pytest.mark.parametrize("way", ["weight 0", "idx -1", "sqdist above", "sqdist NaN"])
@pytest.mark.parametrize("placement", range(len(regimes.sentinel_placements())))
def test_a_row_that_is_not_counted_influences_nothing(placement, way):
    name, x, y, rows = regimes.sentinel_placements()[placement]
    known, worst = None, 0.0
    for value in regimes.SENTINELS:
        sx, sy, kept = regimes.with_sentinels(x, y, rows, value)
        known = known or regimes.truth(sx[kept], sy[kept], None, True, False)
        got = _without(way, sx, sy, kept)
        worst = max(worst, float(np.abs(_n(got.R) - known[0].R).max()))
        print("%s, %s, %g: |R - R64| = %.3g" % (name, way, value, np.abs(_n(got.R) - known[0].R).max()))
    print("WORST sentinels %s, %s: %.3g" % (name, way, worst))
    for value in regimes.SENTINELS:
        sx, sy, kept = regimes.with_sentinels(x, y, rows, value)
        got = _without(way, sx, sy, kept)
        regimes.check(_n(got.R), _n(got.T), float(got.s), sx[kept], sy[kept], None, True, False, True,
                      (name, way, value), known=known)


def test_icp_cut_off_with_the_outliers_first_and_a_far_first_target():
    """tests/test_alignment_gpu.py's test_icp_cut_off_drops_far_outliers with the 30 outliers in the first rows and a
    target 1e5 away from every match as row 0 of the cloud, at that test's tolerances against the clean run."""
    M, N, degrees, scale, seed, _ = ar.ICP_CLOUD_CASES[1]
    x, y, R = ar.icp_cloud_case(M, N, degrees, scale, seed)
    far = (np.random.default_rng(5).uniform(-1, 1, (30, 3)) + np.array([6.0, -7.0, 8.0])).astype(np.float32)
    dirty = np.concatenate([far, x])
    target = np.concatenate([np.array([[1e5, -1e5, 1e5]], np.float32), y])
    run = lambda a, b: points.iterative_closest_point(_d(a), _d(b), max_iterations=20, estimate_scale=True,
                                                      max_correspondence_distance=0.6)
    clean, got = run(x, y), run(dirty, target)
    for mine, theirs in zip(got.RTs, clean.RTs):
        print("ICP, outliers first: difference to the clean run %.3g" % float((mine - theirs).abs().max()))
    assert bool(got.converged) and bool(clean.converged)
    assert ar.angle_between(clean.RTs.R.cpu().numpy(), R) <= 1e-4
    for mine, theirs in zip(got.RTs, clean.RTs):
        assert float((mine - theirs).abs().max()) <= 1e-6
    assert abs(float(got.rmse) - float(clean.rmse)) <= 1e-6 and int(got.iterations) == int(clean.iterations)


# ---- matches through the idx plane ----------------------------------------------------------------------------------

@pytest.mark.parametrize("gather", [True, False])
def test_matches_through_the_idx_plane(gather):
    case = regimes.gather_case()
    x, target, idx = case["x"], case["target"], case["idx"]
    B, N, M = x.shape[0], x.shape[1], target.shape[1]
    valid = (idx >= 0) & (idx < M)
    matched = np.stack([target[b][np.clip(idx[b], 0, M - 1)] for b in range(B)])
    if gather:
        y, plane = target, idx
    else:   # the matches row by row, the plane only marks rows: any value >= 0 keeps one, and none is used as an index
        y, plane = matched, np.where(valid, np.random.default_rng(3).permutation(N)[None, :], -1).astype(np.int32)
    worst = 0.0
    for use_weights, use_lengths, use_cut in itertools.product((False, True), repeat=3):
        R, T, s, _ = _native.align_solve(
            _d(x), _d(y), _d(case["weights"]) if use_weights else None,
            _d(case["lengths"], torch.int32) if use_lengths else None, idx=_d(plane, torch.int32), gather=gather,
            sqdist=_d(case["sqdist"]) if use_cut else None, max_sqdist=case["max_sqdist"] if use_cut else float("inf"),
            estimate_scale=True)
        for b in range(B):
            kept = valid[b].copy()
            if use_lengths:
                kept &= np.arange(N) < case["lengths"][b]
            if use_cut:
                kept &= case["sqdist"][b] <= np.float32(case["max_sqdist"])
            w = case["weights"][b][kept] if use_weights else None
            assert 100 < kept.sum() < N and not kept[0]
            worst = max(worst, _held(R[b], T[b], s[b], x[b][kept], matched[b][kept], w, True, False, True,
                                     "gather=%s %s image %d" % (gather, (use_weights, use_lengths, use_cut), b)))
    print("WORST gather=%s: %.3g" % (gather, worst))


# ---- launch shapes --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,length", [(8193, 8193), (20000, 19000)])
def test_many_chunks_and_a_short_image_in_one_batch(N, length):
    long_x, long_y = regimes.noisy_cloud(N, 41)
    short_x, short_y = regimes.noisy_cloud(300, 42)
    rng = np.random.default_rng(43)
    weights = (rng.integers(0, 256, (2, N)) * (rng.uniform(0, 1, (2, N)) > 0.1)).astype(np.float32) / 256
    x, y = np.full((2, N, 3), np.nan, np.float32), np.full((2, N, 3), np.nan, np.float32)
    x[0, :length], y[0, :length] = long_x[:length], long_y[:length]
    x[1, :300], y[1, :300] = short_x, short_y
    lengths = _d(np.array([length, 300]), torch.int32)
    worst = 0.0
    for use_weights in (False, True):
        w = weights if use_weights else None
        got = points.corresponding_points_alignment(_d(x), _d(y), None if w is None else _d(w), lengths,
                                                    estimate_scale=True)
        for b, n in enumerate((length, 300)):
            worst = max(worst, _held(got.R[b], got.T[b], got.s[b], x[b, :n], y[b, :n], None if w is None else w[b, :n],
                                     True, False, True, "N = %d, weights %s, image %d" % (N, use_weights, b)))
        one = points.corresponding_points_alignment(_d(short_x), _d(short_y), None if w is None else _d(w[1, :300]),
                                                    estimate_scale=True)
        assert torch.equal(one.R, got.R[1]) and torch.equal(one.T, got.T[1]) and torch.equal(one.s, got.s[1])
    print("WORST N = %d: %.3g" % (N, worst))


def test_apply_past_its_grid():
    """2^20 + 300 rows: k_align_apply's grid stops at 4096 workgroups of 256 and strides.  |xt| < 4, so the bound of
    test_unbatched_inputs_and_native_rmse carries over: five float32 roundings of at most half an ulp there (2.4e-7
    each), and R, T, s exact here."""
    N = (1 << 20) + 300
    x = np.random.default_rng(8).uniform(-1, 1, (1, N, 3)).astype(np.float32)
    R = ar.rotation(regimes.AXIS, 25.0).T.astype(np.float32)
    T, s = regimes.SHIFT.astype(np.float32), np.float32(regimes.SCALE)
    xt = _native.align_apply(_d(x), _d(R)[None], _d(T)[None], _d(s).reshape(1),
                             torch.tensor([N - 7], device=DEV, dtype=torch.int32)).cpu().numpy()
    want = float(s) * x[0, :N - 7].astype(np.float64) @ R.astype(np.float64) + T.astype(np.float64)
    assert np.abs(want).max() < 4
    print("apply at N = 2^20 + 300: worst error %.3g" % np.abs(xt[0, :N - 7] - want).max())
    assert np.abs(xt[0, :N - 7] - want).max() <= 3e-6
    assert xt.shape == (1, N, 3) and not xt[0, N - 7:].any()
