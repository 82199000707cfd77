"""numpy float64 restatement of mesh_renderer.points.corresponding_points_alignment and iterative_closest_point: the
definition with numpy.linalg.svd, and the ICP rounds with a brute-force search.  The truth of tests/test_alignment_*;
imports nothing from the package.  Row-vector convention s * x @ R + T ~ y."""
import collections

import numpy as np

Transform = collections.namedtuple("Transform", ["R", "T", "s"])
ICP = collections.namedtuple("ICP", ["converged", "rmse", "Xt", "R", "T", "s", "iterations", "gaps", "matches"])


def alignment(x, y, weights=None, estimate_scale=False, allow_reflection=False):
    """One image: x, y [N,3] (any N >= 0), weights [N] or None -> (Transform, mean squared residual, sigma [3])."""
    x, y = np.asarray(x, np.float64).reshape(-1, 3), np.asarray(y, np.float64).reshape(-1, 3)
    w = np.ones(len(x)) if weights is None else np.asarray(weights, np.float64)
    identity = Transform(np.eye(3), np.zeros(3), 1.0)
    W = w.sum()
    if np.isnan(W) or not (np.isfinite(x[w == w]).all() and np.isfinite(y[w == w]).all() and np.isfinite(w).all()):
        nan = np.full(3, np.nan)
        return Transform(np.full((3, 3), np.nan), nan, np.nan), np.nan, nan
    if not W > 0:
        return identity, 0.0, np.zeros(3)
    xm, ym = (w[:, None] * x).sum(0) / W, (w[:, None] * y).sum(0) / W
    xc, yc = x - xm, y - ym
    C = (w[:, None, None] * xc[:, :, None] * yc[:, None, :]).sum(0) / W
    var_x = (w * (xc * xc).sum(-1)).sum() / W
    if np.abs(C).max() == 0:
        U, S, Vt = np.eye(3), np.zeros(3), np.eye(3)
    else:
        U, S, Vt = np.linalg.svd(C)
    E = np.ones(3)
    if not allow_reflection and np.linalg.det(U @ Vt) < 0:
        E[2] = -1.0
    R = (U * E) @ Vt
    s = float((S * E).sum() / var_x) if estimate_scale and var_x > 0 else 1.0
    T = ym - s * xm @ R
    residual = s * xc @ R - yc
    mse = float((w * (residual * residual).sum(-1)).sum() / W)
    return Transform(R, T, s), mse, S


def residual_of(x, y, transform, weights=None):
    """The weighted mean squared residual of a transform on matched x, y [N,3]."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    w = np.ones(len(x)) if weights is None else np.asarray(weights, np.float64)
    r = transform.s * x @ np.asarray(transform.R, np.float64) + np.asarray(transform.T, np.float64) - y
    return float((w * (r * r).sum(-1)).sum() / w.sum())


def nearest_cloud(xt, y):
    """Brute force: -> (squared distances [N], indices [N], the smallest relative gap between the nearest and the
    second-nearest squared distance over the queries; inf with fewer than two targets)."""
    d = ((xt[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    idx = d.argmin(1)
    best = d[np.arange(len(xt)), idx]
    gap = np.inf
    if y.shape[0] > 1 and len(xt):
        second = np.partition(d, 1, axis=1)[:, 1]
        gap = float(((second - best) / np.maximum(second, 1e-300)).min())
    return best, idx, gap


def icp(x, y=None, closest_point=None, init=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False,
        allow_reflection=False, max_correspondence_distance=None):
    """One image: x [N,3] against the cloud y [M,3], or against a surface given as closest_point(points [N,3]) ->
    (closest points [N,3], squared distances [N]).  The rounds of the interface, in float64."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    R, T, s = (np.eye(3), np.zeros(3), 1.0) if init is None else (np.asarray(init[0], np.float64),
                                                                 np.asarray(init[1], np.float64), float(init[2]))
    converged, rmse, prev, iterations, gaps, matches = False, 0.0, None, 0, [], None
    for _ in range(max_iterations):
        xt = s * x @ R + T
        if y is not None:
            target = np.asarray(y, np.float64).reshape(-1, 3)
            if len(target) and len(x):
                sqdist, idx, gap = nearest_cloud(xt, target)
                gaps.append(gap)
                match, kept, matches = target[idx], np.ones(len(x), bool), idx
            else:
                match, kept, sqdist = np.zeros_like(x), np.zeros(len(x), bool), np.zeros(len(x))
        else:
            match, sqdist = closest_point(xt)
            kept = np.ones(len(x), bool)
        if max_correspondence_distance is not None:
            kept = kept & (sqdist <= float(max_correspondence_distance) ** 2)
        iterations += 1
        if not kept.any():
            converged, rmse = True, 0.0
            break
        (R, T, s), mse, _ = alignment(x[kept], match[kept], None, estimate_scale, allow_reflection)
        rmse = float(np.sqrt(max(mse, 0.0)))
        if rmse == 0 or (iterations >= 2 and (prev - rmse) / prev <= relative_rmse_thr):
            converged = True
            break
        prev = rmse
    return ICP(converged, rmse, s * x @ R + T, R, T, s, iterations, gaps, matches)


def mesh_closest_point(vertices, triangles):
    """-> closest_point(points [N,3]) for icp(): the closest point of the nearest triangle by
    tests/point_mesh_reference.py's float64 definition (brute force over the triangles)."""
    import torch

    import point_mesh_reference as pmref
    v, t = torch.as_tensor(np.asarray(vertices, np.float64))[None], torch.as_tensor(np.asarray(triangles, np.int64))

    def closest_point(points):
        p = torch.as_tensor(np.asarray(points, np.float64))[None]
        sqdist, face = pmref.nearest(p, v, t)
        _, bary = pmref.distance_to_face(p, v, t, face)
        corners = pmref._corners(v, t, face)
        return (bary[..., None] * corners).sum(2)[0].numpy(), sqdist[0].numpy()
    return closest_point


def rotation(axis, degrees):
    """The rotation matrix about `axis` by `degrees` (Rodrigues), for column vectors; use its transpose on rows."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def angle_between(Ra, Rb):
    """The angle in degrees of the rotation Ra^T Rb."""
    c = (np.trace(np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)) - 1.0) / 2.0
    d = np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)
    skew = np.linalg.norm([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]]) / 2.0   # sin, exact near 0
    return float(np.rad2deg(np.arctan2(skew, c)))


ALIGNMENT_SHAPES = [(1, 1), (1, 3), (3, 63), (2, 257), (1, 5000), (64, 300)]
_alignment_cases = {}


def alignment_case(k):
    """Shape k of ALIGNMENT_SHAPES, seeded and built once -> dict of float32 arrays: x [B,N,3] uniform in [-1,1]^3,
    y = a per-image similarity of x (8..40 degrees, scale 0.8..1.25, a shift) plus noise of 0.02, weights [B,N] in
    [0,1) with some exact zeros, lengths [B] int32 in [0, N] (the first image full, the last -- of three or more --
    empty)."""
    if k not in _alignment_cases:
        B, N = ALIGNMENT_SHAPES[k]
        rng = np.random.default_rng(500 + k)
        x = rng.uniform(-1, 1, (B, N, 3))
        y = np.empty_like(x)
        for b in range(B):
            R = rotation(rng.standard_normal(3), rng.uniform(8, 40)).T
            y[b] = rng.uniform(0.8, 1.25) * x[b] @ R + rng.uniform(-0.5, 0.5, 3) + 0.02 * rng.standard_normal((N, 3))
        weights = rng.uniform(0, 1, (B, N)) * (rng.uniform(0, 1, (B, N)) > 0.1)
        lengths = rng.integers(min(4, N), N + 1, B)
        lengths[0] = N
        if B >= 3:
            lengths[-1] = 0
        _alignment_cases[k] = dict(x=x.astype(np.float32), y=y.astype(np.float32), weights=weights.astype(np.float32),
                                   lengths=lengths.astype(np.int32))
    return _alignment_cases[k]


def alignment_batch(x, y, weights=None, lengths=None, estimate_scale=False, allow_reflection=False):
    """alignment() image by image over the valid rows -> (R [B,3,3], T [B,3], s [B], mse [B], sigma [B,3])."""
    out = []
    for b in range(len(x)):
        n = len(x[b]) if lengths is None else int(np.clip(lengths[b], 0, len(x[b])))
        w = None if weights is None else weights[b][:n]
        t, mse, sigma = alignment(x[b][:n], y[b][:n], w, estimate_scale, allow_reflection)
        out.append((t.R, t.T, t.s, mse, sigma))
    return tuple(np.stack([np.asarray(o[k], np.float64) for o in out]) for k in range(5))


def icp_cloud_case(M, N, degrees, scale, seed=0):
    """The planted ICP case of the tests: y = M uniform points in [-1,1]^3; x = the first N moved back by a known
    similarity (rotation by `degrees` about (1,2,3), the shift (0.05,-0.03,0.04), `scale`), rounded to float32, so
    that the true match of x[i] is i.  -> (x [N,3] float32, y [M,3] float32, R [3,3] with s * x @ R + T = y)."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    R = rotation([1, 2, 3], degrees).T
    T = np.array([0.05, -0.03, 0.04])
    x = ((y[:N].astype(np.float64) - T) @ R.T / scale).astype(np.float32)
    return x, y, R


# (M, N, degrees, scale, seed, the rounds within which the float64 loop converges).  The seeds were chosen for the gap
# between the nearest and the second-nearest target, which test_alignment_host.py asserts at every round.
ICP_CLOUD_CASES = [(400, 150, 5.0, 1.0, 0, 3), (400, 150, 8.0, 1.05, 1, 4), (400, 150, 12.0, 1.0, 1, 5),
                   (1000, 257, 5.0, 1.05, 1, 4)]


def cube_mesh():
    """The 8 vertices and 12 triangles of the cube [-1,1]^3 (float64, int64)."""
    v = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = np.array([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], np.int64)
    return v, t


def cube_scan(count, degrees, scale=1.05, seed=0):
    """examples/register_scan.py's configuration: `count` points on the cube's surface (a face and two uniforms per
    point), moved back by a known similarity (rotation by `degrees` about (1,2,3), the shift (0.1,-0.05,0.08),
    `scale`), float32.  -> (scan [count,3] float32, R [3,3], T [3], scale) with scale * scan @ R + T on the cube."""
    rng = np.random.default_rng(seed)
    face, u = rng.integers(0, 6, count), rng.uniform(-1, 1, (count, 2))
    axis, sign = face // 2, (face % 2) * 2.0 - 1.0
    p = np.zeros((count, 3))
    for k in range(count):
        others = [a for a in range(3) if a != axis[k]]
        p[k, axis[k]] = sign[k]
        p[k, others] = u[k]
    R = rotation([1, 2, 3], degrees).T
    T = np.array([0.1, -0.05, 0.08])
    return ((p - T) @ R.T / scale).astype(np.float32), R, T, scale
