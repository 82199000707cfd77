"""Restatement of mesh_renderer.points.sample_farthest_points, written from its definition, and the seeded clouds the
host and the GPU tests share.

  start:     idx[b,0] = start_idx[b] clamped to [0, length_b), 0 by default
  distance:  every valid point carries m_i, +inf at first (0 for a point with a non-finite coordinate, which is never
             updated and as a selected point moves nobody)
  update:    after point s is selected  d_i = ((dx dx) + (dy dy)) + (dz dz), dx = x_i - x_s, each operation rounded on
             its own in this order;  m_i <- d_i if d_i < m_i;  m_s <- -1
  next:      the largest m_i, the lowest index among equals
  radius:    m of the selected point when it is selected, +inf in slot 0; slots k >= length_b: idx -1, radius 0

fps32 does this in numpy float32 and is the bit-exact yardstick of the float32 paths; fps64 is the same on the inputs
promoted to float64.  greedy_shortfall holds a result to the float64 definition without either: by how much, relative,
the point selected at a step falls short of the point that was farthest in float64 from the selections before it."""
import numpy as np
import torch

import points_reference as pref

# (B, N) of cloud k, seeded numpy.random.default_rng(300 + k)
SHAPES = [(1, 1), (1, 2), (3, 63), (2, 65), (2, 257), (1, 1025), (2, 5000), (1, 40000)]
MAX_K = 256

_clouds = {}
_results = {}


def cloud(k):
    """-> [B,N,3] float32 host tensor of shape k (or "translated": points_reference's cloud at offset (100, -50, 25)),
    built once."""
    if k not in _clouds:
        if k == "translated":
            _clouds[k] = pref.translated_clouds()[0]
        else:
            B, N = SHAPES[k]
            rng = np.random.default_rng(300 + k)
            _clouds[k] = torch.from_numpy(rng.uniform(-1, 1, (B, N, 3)).astype(np.float32))
    return _clouds[k]


CASES = list(range(len(SHAPES))) + ["translated"]


def _fps(points, K, lengths, start_idx, dtype):
    p = np.asarray(points, dtype=np.float32).astype(dtype)
    B, N, _ = p.shape
    idx = np.full((B, K), -1, dtype=np.int64)
    radius = np.zeros((B, K), dtype=dtype)
    for b in range(B):
        n = N if lengths is None else int(min(max(int(lengths[b]), 0), N))
        if n == 0:
            continue
        x, y, z = p[b, :n, 0], p[b, :n, 1], p[b, :n, 2]
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        m = np.where(finite, dtype(np.inf), dtype(0))
        s = 0 if start_idx is None else int(min(max(int(start_idx[b]), 0), n - 1))
        r = dtype(np.inf)
        for k in range(min(K, n)):
            idx[b, k], radius[b, k] = s, r
            if finite[s]:
                with np.errstate(over="ignore", invalid="ignore"):
                    dx, dy, dz = x - x[s], y - y[s], z - z[s]
                    d = (dx * dx + dy * dy) + dz * dz
                    closer = finite & (d < m)
                m = np.where(closer, d, m)
            m[s] = dtype(-1)
            s = int(np.argmax(m))          # numpy: the first of equal maxima
            r = m[s]
    return idx, radius


def fps32(points, K, lengths=None, start_idx=None):
    """-> (idx [B,K] int64, radius [B,K] float32) numpy arrays: the definition in float32."""
    return _fps(points, K, lengths, start_idx, np.float32)


def fps64(points, K, lengths=None, start_idx=None):
    """-> (idx [B,K] int64, radius [B,K] float64): the definition on the float32 inputs promoted to float64."""
    return _fps(points, K, lengths, start_idx, np.float64)


def cached_fps32(k):
    """fps32 of cloud k at K = min(N, MAX_K), computed once."""
    if k not in _results:
        c = cloud(k)
        _results[k] = fps32(c.numpy(), min(c.shape[1], MAX_K))
    return _results[k]


def greedy_shortfall(points, idx):
    """points [B,N,3], idx [B,K] (every entry a valid index) -> the worst, over clouds and steps k >= 1, of
    (max_i m_i - m_idx[k]) / max_i m_i  with m_i the float64 squared distance of point i to the nearest of
    idx[0..k-1]: 0 for a result that is greedy in float64 at every step.  A step whose maximum is 0 counts 0."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    idx = np.asarray(idx)
    worst = 0.0
    for b in range(p.shape[0]):
        m = np.full(p.shape[1], np.inf)
        for k in range(1, idx.shape[1]):
            diff = p[b] - p[b, idx[b, k - 1]]
            m = np.minimum(m, (diff * diff).sum(-1))
            m[idx[b, :k]] = -1.0
            best = m.max()
            if best > 0 and np.isfinite(best):
                worst = max(worst, float((best - m[idx[b, k]]) / best))
    return worst
