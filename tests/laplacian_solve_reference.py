"""Helpers of the Laplacian solve's tests (mesh_renderer.preconditioning, csrc/mesh_solve.hip): numpy on the CPU.

Meshes.  sphere8 / sphere25: shapes.sphere(1, K), 66 and 627 vertices, as the library builds them.  strip(V):
triangles (i, i + 1, i + 2), no triangle below V = 3.  fan(V): vertex 0 is a hub of degree V - 1.  strays: sphere8
plus two isolated vertices and one triangle with an index outside the mesh (which mesh_topology drops whole).

Truth.  System64 builds A = I + lam (D - Adj) from the triangles' sides directly -- it never sees mesh_topology --
and solves in float64: dense up to 3000 vertices, above that a float64 CG run to a TRUE residual of 1e-12 |b|.
Since the smallest eigenvalue of A is 1, |x - x*| <= |b - A x| for any x: a truth certifies itself by its own
residual, and truth() asserts it.

Restatement.  cg32 is the algorithm of mesh_renderer/preconditioning.py in float32 vectors and float64 scalars, with
numpy's summation orders and every row of A p in plain float32 (the library evaluates a row in float64 and rounds it
once, which only brings it closer to the truth: cg32 is the yardstick, not a copy).  Its own error |x32 - x64| / |b| per system is what the device's bound is made of
(tests/test_laplacian_solve_gpu.py: max(tol, 4 x this)); tests/test_laplacian_solve_host.py prints it for every case
the device tests use.  Recorded there (tol 1e-6, max over the channels C = 1..4; iterations are the most any system
of the row took):

    mesh      lam   smooth    noise     delta     iterations
    sphere8     0   0         0         0           1
    sphere8     1   1.7e-07   2.4e-07   1.8e-07    18
    sphere8    19   9.4e-08   2.2e-07   2.4e-08    27
    sphere8   100   7.5e-07   8.4e-07   1.7e-07    29
    sphere25    0   0         0         0           1
    sphere25    1   3.5e-07   4.6e-07   3.7e-07    21
    sphere25   19   5.1e-07   8.7e-08   4.9e-08    60
    sphere25  100   2.6e-07   3.5e-08   3.9e-08    73
    fan300      0   0         0         0           1
    fan300      1   2.3e-07   1.8e-07   1.7e-07    13
    fan300     19   1.7e-07   4e-07     2.9e-06    20
    fan300    100   6.6e-07   2.4e-06   4.2e-06    29
    strays      0   0         0         0           1
    strays      1   1.6e-07   2.8e-07   1.8e-07    18
    strays     19   1.1e-07   1.3e-07   2.4e-08    27
    strays    100   6.9e-07   5e-07     1.7e-07    29
"""
import functools

import numpy as np
import torch

from pytorch_mesh_renderer_amd.common import shapes

TOL = 1e-6
MAX_ITERATIONS = 300
LAMBDAS = (0.0, 1.0, 19.0, 100.0)
CHANNELS = (1, 2, 3, 4)
MESHES = ("sphere8", "sphere25", "fan300", "strays")
RIGHT_HAND_SIDES = ("smooth", "noise", "delta")
DENSE_LIMIT = 3000


def strip(V):
    """-> (vertices [V,3] float32, triangles [max(V - 2, 0), 3] int32)."""
    rng = np.random.default_rng(7000 + V)
    at = np.arange(V, dtype=np.float64)
    vertices = np.stack([0.01 * at, np.sin(0.3 * at), np.cos(0.2 * at)], 1) + 0.1 * rng.standard_normal((V, 3))
    i = np.arange(max(V - 2, 0))
    return vertices.astype(np.float32), np.stack([i, i + 1, i + 2], 1).astype(np.int32).reshape(-1, 3)


def fan(V):
    rng = np.random.default_rng(8000 + V)
    angle = np.linspace(0.0, 2.0 * np.pi, V - 1, endpoint=False)
    rim = np.stack([np.cos(angle), np.sin(angle), 0.2 * np.sin(5 * angle)], 1)
    vertices = np.concatenate([np.zeros((1, 3)), rim]) + 0.05 * rng.standard_normal((V, 3))
    i = np.arange(1, V - 1)
    return vertices.astype(np.float32), np.stack([np.zeros_like(i), i, i + 1], 1).astype(np.int32)


def _sphere(K):
    vertices, triangles, _ = shapes.sphere(1.0, K)
    return vertices.numpy().astype(np.float32), triangles.numpy().astype(np.int32)


@functools.lru_cache(maxsize=None)
def mesh(kind):
    """-> (vertices [V,3] float32, triangles [T,3] int32), numpy; do not modify."""
    if kind == "sphere8":
        return _sphere(8)
    if kind == "sphere25":
        return _sphere(25)
    if kind == "fan300":
        return fan(300)
    if kind == "strays":
        vertices, triangles = _sphere(8)
        V = vertices.shape[0]
        vertices = np.concatenate([vertices, np.array([[2.0, 0.5, -1.0], [-1.5, 2.5, 0.25]], np.float32)])
        triangles = np.concatenate([triangles, np.array([[0, 1, V + 2]], np.int32)])   # V + 2: outside the V + 2 vertices
        return vertices, triangles
    if kind.startswith("strip"):
        return strip(int(kind[5:]))
    raise KeyError(kind)


def edges_of(triangles, V):
    """The unique undirected edges [E,2] of the triangles' sides: a triangle with an index outside [0, V) gives none,
    nor does a side whose two ends are the same vertex."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    t = t[((t >= 0) & (t < V)).all(1)]
    pairs = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    pairs = np.sort(pairs[pairs[:, 0] != pairs[:, 1]], 1)
    return np.unique(pairs, axis=0).reshape(-1, 2)


class System64:
    """A = I + lam (D - Adj) in float64.  table [V, max degree]: every vertex's neighbours in ascending order, -1
    beyond its degree -- the order in which neighbour_sum adds them, one float operation after the other."""

    def __init__(self, triangles, V, lam):
        self.V, self.lam = int(V), float(lam)
        edges = edges_of(triangles, V)
        src = np.concatenate([edges[:, 0], edges[:, 1]])
        dst = np.concatenate([edges[:, 1], edges[:, 0]])
        order = np.lexsort((dst, src))
        self.src, self.dst = src[order], dst[order]
        degree = np.bincount(self.src, minlength=self.V)
        self.degree = degree.astype(np.float64)
        self.diagonal = 1.0 + self.lam * self.degree
        first = np.cumsum(degree) - degree
        self.table = np.full((self.V, int(degree.max()) if self.src.size else 0), -1, np.int64)
        self.table[self.src, np.arange(self.src.size) - first[self.src]] = self.dst

    def neighbour_sum(self, x):
        """sum_j x_j over every row's neighbours in ascending j, in x's dtype."""
        sums = np.zeros_like(x)
        zero = x.dtype.type(0)
        for k in range(self.table.shape[1]):
            column = self.table[:, k]
            have = (column >= 0).reshape((-1,) + (1,) * (x.ndim - 1))
            sums += np.where(have, x[np.maximum(column, 0)], zero)
        return sums

    def __matmul__(self, x):
        x = np.asarray(x, np.float64)
        return self.diagonal.reshape((-1,) + (1,) * (x.ndim - 1)) * x - self.lam * self.neighbour_sum(x)

    def absolute(self, x):
        """(|A| |x|)_i = (1 + lam deg_i) |x_i| + lam sum |x_j|."""
        x = np.abs(np.asarray(x, np.float64))
        return self.diagonal.reshape((-1,) + (1,) * (x.ndim - 1)) * x + self.lam * self.neighbour_sum(x)

    def dense(self):
        A = np.diag(self.diagonal)
        A[self.src, self.dst] -= self.lam
        return A

    def solve(self, b):
        """b [V,n] float64 -> x [V,n], certified: |b - A x| <= 1e-12 |b| per column, hence |x - x*| too."""
        b = np.asarray(b, np.float64)
        if self.V <= DENSE_LIMIT:
            x = np.linalg.solve(self.dense(), b)
            x = x + np.linalg.solve(self.dense(), b - self @ x)   # one step of refinement
        else:
            x = self._cg64(b)
        residual = np.linalg.norm(b - self @ x, axis=0)
        assert np.all(residual <= 1e-12 * np.linalg.norm(b, axis=0)), residual
        return x

    def _cg64(self, b):
        x = np.zeros_like(b)
        r = b.copy()
        z = r / self.diagonal[:, None]
        p, rho = z.copy(), (r * z).sum(0)
        goal = 0.5e-12 * np.linalg.norm(b, axis=0)
        for k in range(5000):
            if k % 8 == 0 and np.all(np.linalg.norm(b - self @ x, axis=0) <= goal):
                break
            q = self @ p
            alpha = rho / (p * q).sum(0)
            x += alpha * p
            r -= alpha * q
            z = r / self.diagonal[:, None]
            new = (r * z).sum(0)
            p = z + (new / rho) * p
            rho = new
        return x


@functools.lru_cache(maxsize=None)
def system64(kind, lam):
    vertices, triangles = mesh(kind)
    return System64(triangles, vertices.shape[0], lam)


def pole(kind):
    """The vertex of the highest degree: a pole of the sphere, the hub of the fan."""
    return int(np.argmax(system64(kind, 1.0).degree))


@functools.lru_cache(maxsize=None)
def right_hand_side(kind, which, C):
    """-> [V,C] float32; do not modify."""
    vertices, _ = mesh(kind)
    V = vertices.shape[0]
    if which == "smooth":
        columns = np.concatenate([vertices, vertices.sum(1, keepdims=True) + 0.5], 1)
        return np.ascontiguousarray(columns[:, :C])
    if which == "noise":
        return np.random.default_rng(31 * V + C).standard_normal((V, C)).astype(np.float32)
    if which == "delta":
        b = np.zeros((V, C), np.float32)
        b[pole(kind)] = np.arange(1, C + 1, dtype=np.float32) * np.float32(0.75)
        return b
    raise KeyError(which)


def batch(kind, C):
    """-> [3,V,C] float32: one image per right-hand side."""
    return np.stack([right_hand_side(kind, which, C) for which in RIGHT_HAND_SIDES])


def truth(kind, lam, b):
    """b [B,V,C] -> x [B,V,C] float64."""
    b = np.asarray(b, np.float64)
    B, V, C = b.shape
    x = system64(kind, lam).solve(b.transpose(1, 0, 2).reshape(V, B * C))
    return x.reshape(V, B, C).transpose(1, 0, 2)


def cg32(system, b, tol=TOL, max_iterations=MAX_ITERATIONS, x0=None):
    """The algorithm in float32 vectors and float64 scalars on b [V,n] float32 -> (x [V,n] float32, iterations [n],
    residual [n]).  Every column is a system of its own."""
    f32 = np.float32
    b = np.asarray(b, f32)
    V, n = b.shape
    lam = f32(system.lam)
    diagonal = (1.0 + system.lam * system.degree).astype(f32)[:, None]
    inverse = f32(1.0) / diagonal

    def apply(v):
        return diagonal * v - lam * system.neighbour_sum(v)

    def dot(a, c):
        return (a.astype(np.float64) * c.astype(np.float64)).sum(0)

    x = np.zeros_like(b) if x0 is None else np.asarray(x0, f32).copy()
    r = b.copy() if x0 is None else b - apply(x)
    z = r * inverse
    p, rho = z.copy(), dot(r, z)
    bb, rr = dot(b, b), dot(r, r)
    tol2 = float(tol) ** 2
    poisoned = ~(np.isfinite(bb) & np.isfinite(rr))
    frozen = poisoned | (rr <= tol2 * bb)
    iterations = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for _ in range(max_iterations):
            if frozen.all():
                break
            q = apply(p)
            pq = dot(p, q)
            frozen = frozen | ~((pq > 0) & np.isfinite(pq))
            runs = ~frozen
            alpha = np.where(runs, rho / pq, 0.0).astype(f32)
            x = np.where(runs, x + alpha * p, x)
            r = np.where(runs, r - alpha * q, r)
            iterations += runs
            z = r * inverse
            new_rr, new_rho = dot(r, r), dot(r, z)
            beta = np.where(runs, new_rho / rho, 0.0).astype(f32)
            p = np.where(runs, z + beta * p, p)
            rr, rho = np.where(runs, new_rr, rr), np.where(runs, new_rho, rho)
            frozen = frozen | (rr <= tol2 * bb)
        residual = np.where(bb == 0, 0.0, np.sqrt(rr / np.where(bb == 0, 1.0, bb)))
    x = np.where(poisoned, f32(np.nan), x)
    return x, iterations, np.where(poisoned, np.nan, residual)


def relative_error(x, x64, b):
    """|x - x64| / |b| per system of [B,V,C] arrays -> [B,C] (0 where b = 0 and x = x64)."""
    x, x64, b = (np.asarray(a, np.float64) for a in (x, x64, b))
    error = np.linalg.norm(x - x64, axis=1)
    norm = np.linalg.norm(b, axis=1)
    return np.where(norm > 0, error / np.where(norm > 0, norm, 1.0), error)


@functools.lru_cache(maxsize=None)
def case(kind, lam, C):
    """One accuracy case: the batch of the three right-hand sides.  -> dict(b [3,V,C] f32, x64 [3,V,C],
    cg32_error [3,C], cg32_iterations [3,C]); do not modify."""
    b = batch(kind, C)
    B, V, _ = b.shape
    x64 = truth(kind, lam, b)
    x32, iterations, _ = cg32(system64(kind, lam), b.transpose(1, 0, 2).reshape(V, B * C))
    x32 = x32.reshape(V, B, C).transpose(1, 0, 2)
    return dict(b=b, x64=x64, cg32_error=relative_error(x32, x64, b), cg32_iterations=iterations.reshape(B, C))


def bound(cg32_error, tol=TOL):
    """The device's error bound per system: a float32 recurrence that differs from cg32 in its summation orders alone
    gets four times cg32's own error, and never less than the tolerance it was asked for."""
    return np.maximum(tol, 4.0 * np.asarray(cg32_error))


def tensors(kind, device="cpu"):
    vertices, triangles = mesh(kind)
    return torch.from_numpy(vertices).to(device), torch.from_numpy(triangles).to(device)
