"""Float64 restatement of mesh_renderer.points.knn_points, written from its definition: points_reference.distances
(the brute-force N x M difference form on the float32 inputs promoted to float64) and a lexicographic sort on
(distance, index).

  knn:  the K targets j < y_lengths[b] with the smallest (|x_i - y_j|^2, j), ascending; a slot k >= y_lengths[b] and
        every slot of a padded query (i >= x_lengths[b]) give 0 and -1
  gaps: per slot the relative distance gap to the previous and to the next neighbour of the sorted row, the (K+1)-th
        included: where both exceed points_reference.RUNNER_UP_MARGIN two correctly rounded float32 distances cannot
        swap, so the slot's index is decided ("clear")
"""
import numpy as np
import torch

import points_reference as ref

KS = (1, 3, 8, 16, 32)
UNCLEAR_CAP = 1e-3     # of the slots of any (shape, K)

_sorted = {}


def sorted_rows(x, y, y_lengths=None):
    """-> (distances [B,N,M] f64 ascending per row with the targets beyond y_lengths at +inf, order [B,N,M] i64): a
    stable sort, so equal distances keep ascending index."""
    B, M = x.shape[0], y.shape[1]
    mv = ref._valid(y_lengths, B, M)
    d = ref.distances(x, y).masked_fill(torch.arange(M)[None, None, :] >= mv[:, None, None], float("inf")).numpy()
    order = np.argsort(d, axis=2, kind="stable")
    return torch.from_numpy(np.take_along_axis(d, order, axis=2)), torch.from_numpy(order)


def cached_sorted_rows(k):
    """sorted_rows of cloud k of points_reference.SHAPES (or "translated"), computed once."""
    if k not in _sorted:
        x, y = ref.translated_clouds() if k == "translated" else ref.clouds(k)
        _sorted[k] = sorted_rows(x, y)
    return _sorted[k]


def knn(x, y, K, x_lengths=None, y_lengths=None, rows=None):
    """-> (sqdist [B,N,K] f64, idx [B,N,K] i64, gap_prev [B,N,K], gap_next [B,N,K]).  The gaps are relative to the
    slot's own distance; +inf where there is no such neighbour and for a slot without a result."""
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    nv, mv = ref._valid(x_lengths, B, N), ref._valid(y_lengths, B, M)
    d, order = rows if rows is not None else sorted_rows(x, y, y_lengths)
    pad = max(0, K + 1 - M)
    if pad:
        d = torch.cat([d, torch.full((B, N, pad), float("inf"), dtype=torch.float64)], dim=2)
        order = torch.cat([order, torch.zeros(B, N, pad, dtype=torch.int64)], dim=2)
    slot = torch.arange(K)[None, None, :]
    valid = (torch.arange(N)[None, :, None] < nv[:, None, None]) & (slot < mv[:, None, None])
    own, nxt = d[..., :K], d[..., 1:K + 1]
    prev = torch.cat([torch.full((B, N, 1), -float("inf"), dtype=torch.float64), d[..., :K - 1]], dim=2)
    scale = own.clamp(min=1e-300)
    inf = torch.full_like(own, float("inf"))
    gap_prev = torch.where(valid & torch.isfinite(prev), (own - prev) / scale, inf)
    gap_next = torch.where(valid & torch.isfinite(nxt), (nxt - own) / scale, inf)
    return (torch.where(valid, own, torch.zeros_like(own)),
            torch.where(valid, order[..., :K], torch.full_like(order[..., :K], -1)), gap_prev, gap_next)


def clear_slots(gap_prev, gap_next):
    return (gap_prev > ref.RUNNER_UP_MARGIN) & (gap_next > ref.RUNNER_UP_MARGIN)


def distance_to(x, y, idx):
    """[B,N,K] float64: |x_i - y_idx_ik|^2, 0 where idx is -1."""
    B, N, K = idx.shape
    safe = idx.long().clamp(min=0).reshape(B, N * K, 1).expand(-1, -1, 3)
    chosen = torch.gather(y.double(), 1, safe).reshape(B, N, K, 3)
    diff = x.double()[:, :, None, :] - chosen
    return torch.where(idx.long() >= 0, (diff * diff).sum(-1), torch.zeros(idx.shape, dtype=torch.float64))


def knn_gradients(x, y, idx, upstream):
    """The float64 gradients of sum_ik upstream_ik |x_i - y_idx_ik|^2 for the GIVEN indices -> (dx, dy)."""
    xd, yd = x.double().clone().requires_grad_(True), y.double().clone().requires_grad_(True)
    (distance_to(xd, yd, idx) * upstream.double()).sum().backward()
    return xd.grad, yd.grad


def load_example():
    """examples/estimate_scan_normals.py as a module."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("estimate_scan_normals",
                                                  os.path.join(root, "examples", "estimate_scan_normals.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    return example
