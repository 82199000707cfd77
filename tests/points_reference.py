"""Float64 restatement of mesh_renderer.points, written from its formulas: the brute-force N x M form on the float32
inputs promoted to float64, and the seeded clouds the host and the GPU tests share.

  nearest:  sqdist_i = min_j |x_i - y_j|^2 over j < y_lengths[b], idx_i = the first j that attains it; a padded
            query (i >= x_lengths[b]) or an empty target gives 0 and -1
  chamfer:  x_weight * mean_i sqdist(x -> y) + y_weight * mean_j sqdist(y -> x) over the valid points, an empty side
            contributes 0
  sampling: the face whose interval of the cumulative areas holds u0 * total area, barycentrics
            (1 - sqrt(u1), sqrt(u1) (1 - u2), sqrt(u1) u2)
"""
import numpy as np
import torch

# (B, N, M) of cloud k, seeded numpy.random.default_rng(100 + k).  0..6: the issue's list.  7..9: one point above
# queries_per_lane x workgroup size (1 x 256 and 4 x 256) and one above the target tile (256) of nearest_plan.
SHAPES = [(1, 1, 1), (1, 1, 300), (2, 300, 1), (3, 65, 63), (2, 257, 1031), (1, 40, 5000), (2, 1500, 37),
          (1, 257, 257), (2, 1025, 257), (1, 1025, 100)]
RUNNER_UP_MARGIN = 4e-6   # closer than this (relative) two correctly rounded float32 distances may swap

_clouds = {}
_nearest = {}


def clouds(k):
    """-> (x [B,N,3], y [B,M,3]) float32 host tensors of shape k, built once."""
    if k not in _clouds:
        B, N, M = SHAPES[k]
        rng = np.random.default_rng(100 + k)
        x = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
        y = rng.uniform(-1, 1, (B, M, 3)).astype(np.float32)
        _clouds[k] = (torch.from_numpy(x), torch.from_numpy(y))
    return _clouds[k]


def translated_clouds():
    """Shape (1, 500, 700) at offset (100, -50, 25), seed 7: the case the expansion form of the distance fails."""
    if "translated" not in _clouds:
        rng = np.random.default_rng(7)
        offset = np.array([100.0, -50.0, 25.0])
        x = (rng.uniform(-1, 1, (1, 500, 3)) + offset).astype(np.float32)
        y = (rng.uniform(-1, 1, (1, 700, 3)) + offset).astype(np.float32)
        _clouds["translated"] = (torch.from_numpy(x), torch.from_numpy(y))
    return _clouds["translated"]


def lattice_clouds(wide):
    """Exact ties: targets on an integer lattice with coordinates in 0..7, every point twice, in a seeded shuffle;
    queries at the cell centres, each at squared distance 0.75 from eight corners (sixteen targets).  wide: the
    8 x 8 x 8 lattice (1024 targets, 343 queries), else 8 x 4 x 4 (256 targets: one tile, 63 queries)."""
    nx, ny, nz = (8, 8, 8) if wide else (8, 4, 4)
    grid = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    targets = np.concatenate([grid, grid]).astype(np.float32)
    targets = targets[np.random.default_rng(11).permutation(targets.shape[0])]
    cells = np.stack(np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij"), -1)
    queries = (cells.reshape(-1, 3) + 0.5).astype(np.float32)
    return torch.from_numpy(queries)[None], torch.from_numpy(targets)[None]


def _valid(lengths, B, n):
    if lengths is None:
        return torch.full((B,), n, dtype=torch.int64)
    return torch.as_tensor(lengths).long().cpu().clamp(0, n)


def distances(x, y):
    """[B,N,M] float64: |x_i - y_j|^2 in the difference form."""
    diff = x.double()[:, :, None, :] - y.double()[:, None, :, :]
    return (diff * diff).sum(-1)


def nearest(x, y, x_lengths=None, y_lengths=None):
    """-> (sqdist [B,N] f64, idx [B,N] i64, gap [B,N] f64: (runner-up - nearest) / nearest, inf without a runner-up
    or for a row without a neighbour)."""
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    nv, mv = _valid(x_lengths, B, N), _valid(y_lengths, B, M)
    d = distances(x, y)
    d = d.masked_fill(torch.arange(M)[None, None, :] >= mv[:, None, None], float("inf"))
    idx = torch.from_numpy(np.argmin(d.numpy(), axis=2))   # numpy: the first of equal minima
    best = torch.gather(d, 2, idx[..., None])[..., 0]
    rest = d.scatter(2, idx[..., None], float("inf"))
    second = rest.min(dim=2).values if M > 1 else torch.full_like(best, float("inf"))
    valid = (torch.arange(N)[None, :] < nv[:, None]) & (mv > 0)[:, None]
    gap = torch.where(valid & torch.isfinite(second), (second - best) / best.clamp(min=1e-300),
                      torch.full_like(best, float("inf")))
    return (torch.where(valid, best, torch.zeros_like(best)), torch.where(valid, idx, torch.full_like(idx, -1)), gap)


def cached_nearest(k, reverse=False):
    """nearest() of cloud k (y -> x with reverse), computed once."""
    if (k, reverse) not in _nearest:
        x, y = clouds(k)
        _nearest[(k, reverse)] = nearest(y, x) if reverse else nearest(x, y)
    return _nearest[(k, reverse)]


def directed_mean(sqdist, lengths, other_lengths, other_count):
    B, N = sqdist.shape
    nv, mv = _valid(lengths, B, N), _valid(other_lengths, B, other_count)
    mean = sqdist.sum(1) / nv.clamp(min=1).double()
    return torch.where((nv > 0) & (mv > 0), mean, torch.zeros_like(mean))


def chamfer(x, y, x_lengths=None, y_lengths=None, x_weight=1.0, y_weight=1.0):
    """-> [B] float64."""
    xy = directed_mean(nearest(x, y, x_lengths, y_lengths)[0], x_lengths, y_lengths, y.shape[1])
    yx = directed_mean(nearest(y, x, y_lengths, x_lengths)[0], y_lengths, x_lengths, x.shape[1])
    return x_weight * xy + y_weight * yx


def distance_to(x, y, idx):
    """[B,N] float64: |x_i - y_idx_i|^2, 0 where idx is -1."""
    chosen = torch.gather(y.double(), 1, idx.long().clamp(min=0)[..., None].expand(-1, -1, 3))
    diff = x.double() - chosen
    return torch.where(idx.long() >= 0, (diff * diff).sum(-1), torch.zeros(idx.shape, dtype=torch.float64))


def nearest_gradients(x, y, idx, upstream):
    """The float64 gradients of sum_i upstream_i |x_i - y_idx_i|^2 for the GIVEN indices -> (dx, dy)."""
    xd, yd = x.double().clone().requires_grad_(True), y.double().clone().requires_grad_(True)
    (distance_to(xd, yd, idx) * upstream.double()).sum().backward()
    return xd.grad, yd.grad


def chamfer_gradients(x, y, idx_xy, idx_yx, upstream, x_lengths=None, y_lengths=None, x_weight=1.0, y_weight=1.0):
    """The float64 gradients of sum_b upstream_b chamfer_b evaluated with the GIVEN indices of both directions."""
    xd, yd = x.double().clone().requires_grad_(True), y.double().clone().requires_grad_(True)
    xy = directed_mean(distance_to(xd, yd, idx_xy), x_lengths, y_lengths, y.shape[1])
    yx = directed_mean(distance_to(yd, xd, idx_yx), y_lengths, x_lengths, x.shape[1])
    ((x_weight * xy + y_weight * yx) * upstream.double()).sum().backward()
    return xd.grad, yd.grad


def sample(vertices, triangles, uniforms):
    """[V,3], [T,3], [count,3] -> (points [count,3] f64, faces [count], barycentrics [count,3] f64), one sample at a
    time from the formulas."""
    v, tri, u = vertices.double().numpy(), triangles.long().numpy(), uniforms.double().numpy()
    areas = np.array([0.5 * np.linalg.norm(np.cross(v[b] - v[a], v[c] - v[a])) for a, b, c in tri])
    cumulative = np.cumsum(areas)
    points, faces, barys = [], [], []
    for u0, u1, u2 in u:
        value = u0 * cumulative[-1]
        face = next(f for f in range(len(tri)) if cumulative[f] > value)
        root = np.sqrt(u1)
        bary = np.array([1.0 - root, root * (1.0 - u2), root * u2])
        points.append(bary @ v[tri[face]])
        faces.append(face)
        barys.append(bary)
    return torch.tensor(np.array(points)), torch.tensor(faces), torch.tensor(np.array(barys))
