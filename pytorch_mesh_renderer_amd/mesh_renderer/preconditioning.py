"""Laplacian preconditioning of mesh fitting: the change of variables u = (I + lam L) x.

Optimise u instead of the vertices x and recover x = (I + lam L)^-1 u at every step (Nicolet, Jacobson, Jakob:
"Large Steps in Inverse Rendering", 2021): the gradient that reaches the vertices has passed through the inverse and
is smooth by construction, so no regulariser has to pull against the data term ("Preconditioned
optimisation").  L = D - Adj is the combinatorial graph Laplacian of mesh_topology(triangles, V); A = I + lam L is
symmetric positive definite with smallest eigenvalue 1, and a vertex without neighbours has the identity row.

The solve is Jacobi-preconditioned conjugate gradients, and the algorithm is part of the interface.  Every
(image, channel) pair is a system of its own.  With M = diag(1 + lam deg):

    x = x0 or 0,  r = b - A x,  z = r / M,  p = z,  rho = r.z
    per iteration:  q = A p,  alpha = rho / p.q,  x += alpha p,  r -= alpha q,  z = r / M,  rho' = r.z,
                    p = z + (rho' / rho) p

A system freezes -- its x, iterations and residual never change again, bit for bit -- the first time
    1. r.r <= tol^2 b.b            (tested before the first iteration and after every one)
    2. b.b or the initial r.r is not finite: the system's x is NaN, 0 iterations
    3. p.q <= 0 or not finite      (breakdown: the system keeps the x it had)
The dot products, alpha and beta are float64 and meet the vectors rounded once; so is every row of A p.

On a HIP device in float32 both functions run csrc/mesh_solve.hip.  Host tensors and tensors that are not float32
-- gradcheck, the CPU test-suite -- take the same algorithm as a batched torch expression in their own dtype.
"""
import torch

from .. import _native
from .regularizers import _integer_triangles


def _arguments(x, triangles, lam, name):
    """-> (x as [B,V,C], topology, lam, whether x came without the batch axis)."""
    if not torch.is_tensor(x) or not x.is_floating_point():
        raise TypeError("%s must be a floating-point tensor" % name)
    single = x.dim() == 2
    v = x.unsqueeze(0) if single else x
    if v.dim() != 3 or v.shape[0] < 1 or v.shape[1] < 1 or not 1 <= v.shape[2] <= 4:
        raise ValueError("%s must have shape [B, V, C] or [V, C] with V >= 1 and C in 1..4, got %s"
                         % (name, list(x.shape)))
    _integer_triangles(triangles)
    if isinstance(lam, bool) or not isinstance(lam, (int, float)):
        raise TypeError("lam must be a Python number, got %s" % type(lam).__name__)
    lam = float(lam)
    if not 0.0 <= lam < float("inf"):
        raise ValueError("lam must be a finite number >= 0, got %r" % (lam,))
    if triangles.device != v.device:
        triangles = triangles.to(v.device)
    return v, _native.mesh_topology(triangles, v.shape[1]), lam, single


def _native_route(v):
    return v.is_cuda and v.dtype == torch.float32


class _Operator:
    """A of one topology as torch ops on [B,C,V] tensors of one device and dtype.  A row is evaluated in float64 and
    rounded once, like the dot products (in float32 a hub's long row alone costs several times the tolerance)."""

    def __init__(self, topology, lam, like):
        edges = topology.edges.to(like.device).long()
        self.src = torch.cat([edges[:, 0], edges[:, 1]])
        self.dst = torch.cat([edges[:, 1], edges[:, 0]])
        degree = torch.zeros(topology.vertex_count, dtype=torch.float64, device=like.device).index_add_(
            0, self.src, torch.ones(self.src.shape[0], dtype=torch.float64, device=like.device))
        self.lam = lam
        self.diagonal64 = 1.0 + lam * degree
        self.diagonal = self.diagonal64.to(like.dtype)

    def __call__(self, v):
        wide = v.double()
        sums = torch.zeros_like(wide).index_add(2, self.src, wide.index_select(2, self.dst))
        return (self.diagonal64 * wide - self.lam * sums).to(v.dtype)


def _apply_torch(v, topology, lam):
    return _Operator(topology, lam, v)(v.transpose(1, 2)).transpose(1, 2)


def _dot(a, b):
    """[B,C,V] x [B,C,V] -> [B,C] in float64, every system summed over its own contiguous row."""
    return (a.double().contiguous() * b.double().contiguous()).sum(-1)


def _solve_torch(b, topology, lam, tol, max_iterations, x0=None, check_every=0):
    """The algorithm of the module's docstring on [B,V,C] tensors of any device and floating dtype
    -> (x, iterations [B,C] int32, residual [B,C] float32).  On the host every iteration looks whether all systems
    are frozen; on a device only every check_every iterations (0: never)."""
    A = _Operator(topology, lam, b)
    rhs = b.transpose(1, 2).contiguous()
    x = torch.zeros_like(rhs) if x0 is None else x0.to(rhs.dtype).transpose(1, 2).contiguous()
    r = rhs if x0 is None else rhs - A(x)
    inverse = 1.0 / A.diagonal
    bb, rr = _dot(rhs, rhs), _dot(r, r)
    z = r * inverse
    p, rho = z, _dot(r, z)
    tol2 = tol * tol
    poisoned = ~(torch.isfinite(bb) & torch.isfinite(rr))
    frozen = poisoned | (rr <= tol2 * bb)
    iterations = torch.zeros(bb.shape, dtype=torch.int32, device=b.device)
    each = 1 if not b.is_cuda else check_every
    for it in range(max_iterations):
        if each and it % each == 0 and bool(frozen.all()):
            break
        q = A(p)
        pq = _dot(p, q)
        frozen = frozen | ~((pq > 0) & torch.isfinite(pq))
        runs = ~frozen
        alpha = torch.where(runs, rho / pq, torch.zeros_like(pq)).to(rhs.dtype)[..., None]
        x = torch.where(runs[..., None], x + alpha * p, x)
        r = torch.where(runs[..., None], r - alpha * q, r)
        iterations = iterations + runs.to(torch.int32)
        z = r * inverse
        new_rr, new_rho = _dot(r, r), _dot(r, z)
        beta = torch.where(runs, new_rho / rho, torch.zeros_like(rho)).to(rhs.dtype)[..., None]
        p = torch.where(runs[..., None], z + beta * p, p)
        rr, rho = torch.where(runs, new_rr, rr), torch.where(runs, new_rho, rho)
        frozen = frozen | (rr <= tol2 * bb)
    x = torch.where(poisoned[..., None], torch.full_like(x, float("nan")), x)
    residual = torch.where(bb == 0, torch.zeros_like(bb), torch.sqrt(rr / torch.where(bb == 0, torch.ones_like(bb), bb)))
    residual = torch.where(poisoned, torch.full_like(residual, float("nan")), residual)
    return x.transpose(1, 2).contiguous(), iterations, residual.float()


class _Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, topology, lam):
        ctx.topology, ctx.lam = topology, lam
        return _native.laplacian_apply(x.detach().contiguous(), topology, lam)

    @staticmethod
    def backward(ctx, dy):   # A is symmetric
        return _Apply.apply(dy.contiguous(), ctx.topology, ctx.lam), None, None


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, topology, lam, tol, max_iterations, x0, check_every):
        ctx.topology, ctx.settings = topology, (lam, tol, max_iterations, check_every)
        x, iterations, residual = _native.laplacian_solve(
            u.detach().contiguous(), topology, lam, tol, max_iterations,
            None if x0 is None else x0.detach().contiguous(), check_every)
        ctx.mark_non_differentiable(iterations, residual)
        return x, iterations, residual

    @staticmethod
    def backward(ctx, dx, _iterations, _residual):   # the same solve of the incoming gradient, without a start
        lam, tol, max_iterations, check_every = ctx.settings
        du = _Solve.apply(dx.contiguous(), ctx.topology, lam, tol, max_iterations, None, check_every)[0]
        return du, None, None, None, None, None, None


class _SolveTorch(torch.autograd.Function):
    """_solve_torch with the backward of the definition (autograd through the iterations would differentiate the
    freeze decisions' side of the algorithm, not the solve)."""

    @staticmethod
    def forward(ctx, u, topology, lam, tol, max_iterations, x0, check_every):
        ctx.topology, ctx.settings = topology, (lam, tol, max_iterations, check_every)
        with torch.no_grad():
            x, iterations, residual = _solve_torch(u, topology, lam, tol, max_iterations, x0, check_every)
        ctx.mark_non_differentiable(iterations, residual)
        return x, iterations, residual

    @staticmethod
    def backward(ctx, dx, _iterations, _residual):
        lam, tol, max_iterations, check_every = ctx.settings
        du = _SolveTorch.apply(dx, ctx.topology, lam, tol, max_iterations, None, check_every)[0]
        return du, None, None, None, None, None, None


def to_differential(x, triangles, lam):
    """x [B,V,C] (or [V,C]: one image), C in 1..4, triangles [T,3] of any integer dtype, one topology for the batch
    -> u = (I + lam L) x, the same shape.  lam: a finite Python number >= 0.  Differentiable in x (the backward is
    the same product: A is symmetric).  One launch on a HIP device in float32."""
    v, topology, lam, single = _arguments(x, triangles, lam, "x")
    u = _Apply.apply(v, topology, lam) if _native_route(v) else _apply_torch(v, topology, lam)
    return u[0] if single else u


def from_differential(u, triangles, lam, tol=1e-6, max_iterations=300, x0=None, check_every=0, return_info=False):
    """u [B,V,C] (or [V,C]) -> x with (I + lam L) x = u, by the conjugate gradients of the module's docstring.
    tol: relative residual |r| <= tol |u| at which a system freezes; max_iterations in 0..10000; x0: a start of
    u's shape, e.g. the previous step's vertices (it receives no gradient).  Differentiable in u: the backward is
    the same solve of the incoming gradient with the same tol and max_iterations and no x0.  check_every = 0 reads
    nothing back -- the call is capturable in a HIP graph; k > 0 lets the host read one word every k iterations and
    stop launching once every system is frozen (eager only: it raises under stream capture).  return_info: also
    (iterations [B,C] int32, residual [B,C] float32), [C] each for [V,C] input."""
    v, topology, lam, single = _arguments(u, triangles, lam, "u")
    if isinstance(tol, bool) or not isinstance(tol, (int, float)):
        raise TypeError("tol must be a Python number, got %s" % type(tol).__name__)
    tol = float(tol)
    if not 0.0 <= tol < float("inf"):
        raise ValueError("tol must be a finite number >= 0, got %r" % (tol,))
    for name, value in (("max_iterations", max_iterations), ("check_every", check_every)):
        if isinstance(value, bool) or not isinstance(value, int):
            raise TypeError("%s must be an int, got %s" % (name, type(value).__name__))
    if not 0 <= max_iterations <= 10000:
        raise ValueError("max_iterations must lie in 0..10000, got %d" % max_iterations)
    if check_every < 0:
        raise ValueError("check_every must be >= 0, got %d" % check_every)
    if x0 is not None:
        if not torch.is_tensor(x0) or not x0.is_floating_point():
            raise TypeError("x0 must be a floating-point tensor")
        x0 = x0.unsqueeze(0) if single and x0.dim() == 2 else x0
        if x0.shape != v.shape:
            raise ValueError("x0 must have u's shape %s, got %s" % (list(u.shape), list(x0.shape)))
        if x0.device != v.device or x0.dtype != v.dtype:
            raise ValueError("x0 must have u's device and dtype")
        x0 = x0.detach()
    if check_every and v.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("check_every > 0 reads back from the device, which a stream capture cannot do: "
                           "capture the solve with check_every=0")
    if _native_route(v):
        x, iterations, residual = _Solve.apply(v, topology, lam, tol, max_iterations, x0, check_every)
    else:
        x, iterations, residual = _SolveTorch.apply(v, topology, lam, tol, max_iterations, x0, check_every)
    if single:
        x, iterations, residual = x[0], iterations[0], residual[0]
    return (x, iterations, residual) if return_info else x
