"""The regimes of corresponding_points_alignment's solve, as shared cases for tests/test_alignment_truth_*.py: planted
transforms that reach every branch of the determinant correction and of the rank decisions, rows that must influence
nothing, gathered matches, and the check that holds a result to the numpy float64 truth of
tests/alignment_reference.py.  Imports nothing from the package.

A case is (name, x [N,3], y [N,3], weights [N] or None, expects_unique) in float32; expects_unique is the pair
(without reflection, with allow_reflection): whether R is held entry by entry or only through its residual.  With
sigma the singular values of the truth's covariance and e = det(U V^T) (1 with allow_reflection), R = U E V^T is
conditioned by the pair sums sigma_i + sigma_j of which g = sigma_2 + e sigma_3 is the smallest; R counts as unique
when g >= 0.05 sigma_1 and, with reflection allowed, sigma_3 > 1e-6 sigma_1 (a flat cloud's mirror image fits
equally well).  check() asserts that the truth's g agrees with the stated flag, so that no case slides from one
comparison to the other unseen."""
import itertools

import numpy as np

import alignment_reference as ar

EPS = 2.0 ** -23
RESIDUAL_UNITS = 18          # tests/test_alignment_gpu.py's docstring derives both
SCALE = 1.25
SHIFT = np.array([0.25, -0.5, 0.125])
AXIS = [1.0, 2.0, 3.0]
SLAB_EXPONENTS = (8, 12, 16, 18, 20, 21, 22, 23)

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def base_cloud():
    """64 points (one chunk) on a 2^-10 grid in [-1,1]^3 with the axes scaled by (1, 0.7, 0.4): distinct singular
    values, and 1.25 x P + SHIFT is exact in float32 for every signed permutation P."""
    def make():
        u = np.random.default_rng(2024).uniform(-1, 1, (64, 3)) * np.array([1.0, 0.7, 0.4])
        return np.round(u * 1024) / 1024
    return _once("base", make)


def planted(x, M):
    """-> (x, y) float32 with y = 1.25 x M + SHIFT rounded once."""
    x = np.asarray(x, np.float64)
    return x.astype(np.float32), (SCALE * x @ M + SHIFT).astype(np.float32)


def signed_permutations():
    """-> [(name, P)] all 48, the 24 proper ones first."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            P = np.zeros((3, 3))
            P[np.arange(3), perm] = signs
            out.append(("perm %s %s" % ("".join(map(str, perm)), "".join("+" if v > 0 else "-" for v in signs)), P))
    return sorted(out, key=lambda item: -np.linalg.det(item[1]))


MIRROR = np.diag([1.0, 1.0, -1.0])


def regime_cases():
    """Every regime case, built once.  -> list of (name, x, y, weights, (unique, unique with reflection), family)."""
    def make():
        cases = []
        base = base_cloud()
        rot = lambda degrees, axis=AXIS: ar.rotation(axis, degrees).T
        for name, P in signed_permutations():
            cases.append((name,) + planted(base, P) + (None, (True, True), "signed permutations"))
        for degrees in (90.0, 120.0, 179.999, 180.0, 1e-5, 0.0):
            M = np.eye(3) if degrees == 0.0 else rot(degrees)
            cases.append(("rotation %g" % degrees,) + planted(base, M) + (None, (True, True), "general rotations"))
        cases.append(("mirror",) + planted(base, rot(25.0) @ MIRROR) + (None, (True, True), "mirror"))
        w = np.random.default_rng(7).integers(0, 256, 64).astype(np.float32) / 256       # some exact zeros, a 2^-8 grid
        w[:3] = 0.0
        cases.append(("mirror, weighted",) + planted(base, rot(25.0) @ MIRROR) + (w, (True, True), "mirror"))
        cases.append(("rotation 120, weighted",) + planted(base, rot(120.0)) + (w, (True, True), "general rotations"))
        corners = np.array([[a, b, c] for a in (-1.0, 1.0) for b in (-1.0, 1.0) for c in (-1.0, 1.0)])
        cases.append(("cube",) + planted(corners, rot(33.0)) + (None, (True, True), "equal singular values"))
        cases.append(("cube (1,1,0.5)",) + planted(corners * np.array([1.0, 1.0, 0.5]), rot(33.0))
                     + (None, (True, True), "equal singular values"))
        cases.append(("cube mirrored",) + planted(corners, MIRROR @ rot(33.0)) + (None, (False, True),
                                                                                  "equal singular values"))
        flat = base * np.array([1.0, 1.0, 0.0])
        cases.append(("planar",) + planted(flat, rot(33.0)) + (None, (True, False), "planar"))
        cases.append(("planar mirrored in the plane",) + planted(flat, np.diag([1.0, -1.0, 1.0]) @ rot(33.0))
                     + (None, (True, False), "planar"))
        # slabs: z a multiple of 2^-t / 4 within +-2^-t, turned within the plane so that the thin coordinate of y,
        # +-1.25 z + 0.125, is exact in float32 (t = 23 needs even multiples for that) and the third singular value is
        # the slab's own thickness down to 2e-14 sigma_1, not the rounding of y
        steps = np.random.default_rng(11).integers(-4, 5, 64).astype(np.float64)
        for t in SLAB_EXPONENTS:
            z = (np.round(steps / 2) * 2 if t == 23 else steps) * 2.0 ** -(t + 2)
            slab = np.concatenate([base[:, :2], z[:, None]], axis=1)
            for mirrored in (False, True):
                M = rot(33.0, [0.0, 0.0, 1.0]) @ (MIRROR if mirrored else np.eye(3))
                x, y = planted(slab, M)
                assert np.array_equal(y[:, 2].astype(np.float64), (SCALE * slab @ M + SHIFT)[:, 2])
                cases.append(("slab 2^-%d%s" % (t, " mirrored" if mirrored else ""), x, y, None, (True, t == 8), "slabs"))
        return cases
    return _once("regimes", make)


def truth(x, y, w, estimate_scale, reflect):
    """-> (Transform, mse, sigma [3], e, g / sigma_1, unique) of the float64 restatement on float32 arrays."""
    want, mse, sigma = ar.alignment(x, y, w, estimate_scale, reflect)
    free, _, _ = ar.alignment(x, y, w, False, True)                  # U V^T: its determinant is e
    e = 1.0 if reflect or np.linalg.det(free.R) >= 0 else -1.0
    g = sigma[1] + e * sigma[2]
    unique = bool(g >= 0.05 * sigma[0] and (sigma[2] > 1e-6 * sigma[0] or not reflect))
    return want, mse, sigma, e, (g / sigma[0] if sigma[0] > 0 else 0.0), unique


def ulp32(v):
    return np.maximum(np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64), EPS)


def variance(a, w):
    a = np.asarray(a, np.float64)
    mean = np.average(a, axis=0, weights=w)
    return float(np.average(((a - mean) ** 2).sum(-1), weights=w))


def check(R, T, s, x, y, w, estimate_scale, reflect, expects_unique, what, tol=None, known=None):
    """Holds one image's result (R [3,3], T [3], s, anything numpy converts) to the truth on the float32 arrays x, y
    [n,3] (w [n] or None): the rows that count and nothing else.  tol None: the float32 bounds of
    tests/test_alignment_gpu.py -- |R - R64| <= 2^-23, s and T within one float32 ulp (floor 2^-23), orthonormality and
    determinant within 4 x 2^-23 where R is unique; elsewhere the residual within 18 x 2^-24 x (s^2 var x + var y) of
    the minimum and |det| = 1.  tol a number: a float64 result, held to tol throughout.  known: truth() of the same
    arguments where the caller keeps it.  -> |R - R64| where it was asserted, else None."""
    R, T, s = np.asarray(R, np.float64), np.asarray(T, np.float64), float(s)
    want, mse, sigma, e, g, unique = known if known is not None else truth(x, y, w, estimate_scale, reflect)
    assert unique == expects_unique, (what, "g / sigma_1 = %.3g, sigma_3 / sigma_1 = %.3g" % (g, sigma[2] / sigma[0]))
    frame = 4 * EPS if tol is None else tol
    assert np.isfinite(R).all() and np.abs(R @ R.T - np.eye(3)).max() <= frame, what
    det = np.linalg.det(R)
    if unique:
        assert abs(det - np.linalg.det(want.R)) <= frame, (what, det)
        worst = float(np.abs(R - want.R).max())
        assert worst <= (EPS if tol is None else tol), (what, worst)
        assert abs(s - want.s) <= (ulp32(want.s) if tol is None else tol * max(1.0, abs(want.s))), (what, s, want.s)
        assert (np.abs(T - want.T) <= (ulp32(want.T) if tol is None else tol)).all(), (what, T, want.T)
    else:
        worst = None
        assert abs(abs(det) - 1) <= frame and (reflect or det > 0), (what, det)
    mine = ar.residual_of(x, y, ar.Transform(R, T, s), w)
    bound = RESIDUAL_UNITS * 2.0 ** -24 * (want.s ** 2 * variance(x, w) + variance(y, w)) if tol is None else tol
    assert abs(mine - mse) <= bound + 1e-13, (what, mine, mse, bound)
    return worst


def padded_batch(cases):
    """The cases stacked into one batch, NaN in the padding -> (x [B,N,3], y [B,N,3], weights [B,N] (1 where a case
    has none), lengths [B] int32)."""
    N = max(len(c[1]) for c in cases)
    x = np.full((len(cases), N, 3), np.nan, np.float32)
    y = np.full((len(cases), N, 3), np.nan, np.float32)
    w = np.ones((len(cases), N), np.float32)
    for b, c in enumerate(cases):
        x[b, :len(c[1])], y[b, :len(c[1])] = c[1], c[2]
        if c[3] is not None:
            w[b, :len(c[1])] = c[3]
    return x, y, w, np.array([len(c[1]) for c in cases], np.int32)


# ---- rows that must influence nothing -------------------------------------------------------------------------------

SENTINELS = (1e4, 1e6, 3e38)


def noisy_cloud(n, seed):
    """-> (x, y) float32 [n,3]: x uniform in [-1,1]^3, y a similarity of it (20 degrees, 1.1) plus noise of 0.02."""
    def make():
        rng = np.random.default_rng(seed)
        x = rng.uniform(-1, 1, (n, 3))
        y = 1.1 * x @ ar.rotation([2, -1, 1], 20.0).T + np.array([0.2, 0.1, -0.3]) + 0.02 * rng.standard_normal((n, 3))
        return x.astype(np.float32), y.astype(np.float32)
    return _once(("noisy", n, seed), make)


def sentinel_placements():
    """-> [(name, x, y, rows)]: the clouds and the rows that hold sentinels: row 0 of the base cloud (with its mirror
    target), and of a cloud of 2100 rows (three chunks) row 0, row 1024 (the first of chunk 1), rows 2048..2099 (all
    of chunk 2, which then keeps no row), and all of these at once."""
    bx, by = planted(base_cloud(), ar.rotation(AXIS, 25.0).T @ MIRROR)
    x, y = noisy_cloud(2100, 31)
    tail = np.arange(2048, 2100)
    return [("base row 0", bx, by, np.array([0])), ("row 0", x, y, np.array([0])), ("row 1024", x, y, np.array([1024])),
            ("chunk 2", x, y, tail), ("rows 0, 1024 and chunk 2", x, y, np.concatenate([[0, 1024], tail]))]


def with_sentinels(x, y, rows, value):
    """-> copies with x = +value and y = -value in `rows`, and the mask of the other rows."""
    x, y = x.copy(), y.copy()
    x[rows], y[rows] = np.float32(value), -np.float32(value)
    kept = np.ones(len(x), bool)
    kept[rows] = False
    return x, y, kept


# ---- matches read through an idx plane ------------------------------------------------------------------------------

def gather_case():
    """B = 2, N = 300, M = 500: a target cloud, a random map idx with repeats, entries of -1 and entries >= M, and x
    the matched targets moved back by a similarity plus noise; weights, lengths, a sqdist plane with its cut-off.
    -> dict of arrays; `kept(...)` of the options says which rows count."""
    def make():
        rng = np.random.default_rng(99)
        B, N, M = 2, 300, 500
        target = rng.uniform(-1, 1, (B, M, 3)).astype(np.float32)
        idx = rng.integers(0, M, (B, N)).astype(np.int32)
        idx[:, 0] = -1                                               # the first row of the first chunk is dropped
        idx[rng.uniform(0, 1, (B, N)) < 0.1] = -1
        idx[rng.uniform(0, 1, (B, N)) < 0.05] = M
        idx[0, 7], idx[1, 9] = M + 12345, -7
        x = np.empty((B, N, 3), np.float32)
        for b in range(B):
            R = ar.rotation(rng.standard_normal(3), 30.0 + 10 * b).T
            match = target[b][np.clip(idx[b], 0, M - 1)].astype(np.float64)
            x[b] = ((match - np.array([0.1, -0.2, 0.3])) @ R.T / 1.2 + 0.02 * rng.standard_normal((N, 3)))
        weights = (rng.integers(0, 256, (B, N)) * (rng.uniform(0, 1, (B, N)) > 0.1)).astype(np.float32) / 256
        sqdist = rng.uniform(0, 1, (B, N)).astype(np.float32)
        return dict(x=x, target=target, idx=idx, weights=weights, sqdist=sqdist, max_sqdist=0.75,
                    lengths=np.array([300, 211], np.int32))
    return _once("gather", make)
