"""Float64 restatement of mesh_renderer.points.winding_number, written from the definition (INTEGRATION.md,
"Point-cloud losses"), its a-posteriori rounding bound, and the inputs the host and the GPU tests share.

  a = va - p, b = vb - p, c = vc - p;  num = a . (b x c);  den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|
  w = sum over the counted triangles of 2 atan2(num, den) / (4 pi)
evaluated on the float32 inputs promoted to float64 and summed plainly.  A triangle with an index outside [0, V) or
with two equal indices is not counted.

The bound, per query, with M = |a||b||c|, r = hypot(num, den), Omega = 2 atan2(num, den) over the counted triangles:
  E_i = 2^-24 * sum_f (16 * 2 M_f / r_f + 4 |Omega_f|) / (4 pi)  +  T * 2^-41
An error (dn, dd) in (num, den) moves atan2 by at most hypot(dn, dd) / r, and each of num and den is about a dozen
float32 roundings of magnitude <= M: the first term.  The second allows atan2 8 * 2^-24 relative.  The third is the
rounding of every term to a multiple of 2^-40.  With the constant 1 in place of 16 the float32 torch evaluation
reaches 2.9 E on these inputs; with 16 it stays at or below 0.21 E, which leaves the HIP kernels (other fused
multiply-adds, a 1-ulp square root, another atan2) a factor of about 5.
"""
import math

import numpy as np
import torch

import point_mesh_reference as pm
from pytorch_mesh_renderer_amd.common import shapes

SOUPS = [0, 2, 3, 5, 6, 7, 8, "translated"]
OFFSET = (100.0, -50.0, 25.0)
EASY_BOUND = 1e-3       # the bound must not grow until it hides a failure:
EASY_SHARE = 0.9        # at least this share of a case's queries has E_i <= EASY_BOUND

_cases = {}
_truth = {}


def _sphere(offset=None):
    v, t, _ = shapes.sphere_arrays(1.0, 25)
    rng = np.random.default_rng(512)
    p = rng.uniform(-1.5, 1.5, (1, 257, 3))
    p[0, 0] = 0.0   # the centre: 0.96, the sphere is open at the poles' seams
    v = v.astype(np.float64)[None]
    if offset is not None:
        v, p = v + np.asarray(offset), p + np.asarray(offset)
    return (torch.from_numpy(p.astype(np.float32)), torch.from_numpy(v.astype(np.float32)),
            torch.from_numpy(t.astype(np.int64)))


def _cube():
    v, t, _ = shapes.cube(1.0)
    rng = np.random.default_rng(511)
    p = rng.uniform(-1.5, 1.5, (2, 300, 3))
    return torch.from_numpy(p.astype(np.float32)), v[None].repeat(2, 1, 1).contiguous(), t.long()


NAMES = ["soup_%s" % k for k in SOUPS] + ["cube", "sphere", "sphere_translated"]


def case(name):
    """-> (points [B,N,3] f32, vertices [B,V,3] f32, triangles [T,3] i64), built once."""
    if name not in _cases:
        if name.startswith("soup_"):
            k = name[5:]
            _cases[name] = pm.mesh(k if k == "translated" else int(k))
        else:
            _cases[name] = {"cube": _cube, "sphere": _sphere, "sphere_translated": lambda: _sphere(OFFSET)}[name]()
    return _cases[name]


def counted(triangles, V):
    t = triangles.long()
    return ((t >= 0) & (t < V)).all(dim=1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])


def winding(points, vertices, triangles, lengths=None):
    """-> (w [B,N] f64, E [B,N] f64); padded rows 0 / 0."""
    p, v, t = points.double(), vertices.double(), triangles.long()
    B, N = p.shape[:2]
    V, T = v.shape[1], t.shape[0]
    use = counted(t, V)
    safe = t.clamp(0, V - 1)
    w, bound = torch.zeros(B, N, dtype=torch.float64), torch.zeros(B, N, dtype=torch.float64)
    rows = max(1, (1 << 22) // max(1, B * T))
    for s in range(0, N, rows):
        q = p[:, s:s + rows, None, :]
        a, b, c = (v[:, safe[:, k]][:, None] - q for k in range(3))                      # [B,rows,T,3]
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        num = (a * torch.cross(b, c, dim=-1)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        omega = 2.0 * torch.atan2(num, den)
        r = torch.hypot(num, den)
        M = la * lb * lc
        ratio = torch.where(r > 0, M / torch.where(r > 0, r, torch.ones_like(r)), torch.zeros_like(r))
        per = (16.0 * 2.0 * ratio + 4.0 * omega.abs()) / (4.0 * math.pi)
        zero = torch.zeros_like(omega)
        w[:, s:s + rows] = torch.where(use, omega / (4.0 * math.pi), zero).sum(-1)
        bound[:, s:s + rows] = 2.0 ** -24 * torch.where(use, per, zero).sum(-1) + T * 2.0 ** -41
    valid = torch.arange(N)[None, :] < pm._valid(lengths, B, N)[:, None]
    return torch.where(valid, w, torch.zeros_like(w)), torch.where(valid, bound, torch.zeros_like(bound))


def truth(name):
    """winding(*case(name)), computed once and shared."""
    if name not in _truth:
        _truth[name] = winding(*case(name))
    return _truth[name]


def check(got, want, bound, what):
    """Every query within its own E_i, the worst err / E printed first; -> that ratio."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), "%s: a result is not finite" % what
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)), err * float("inf"))
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    share = float((bound <= EASY_BOUND).double().mean())
    worst = float(ratio.max())
    print("%s: worst err/E %.3f (err %.3g), share of queries with E <= 1e-3: %.3f" % (what, worst, float(err.max()), share))
    assert share >= EASY_SHARE, "%s: the bound is loose on %.3f of the queries" % (what, 1 - share)
    assert worst <= 1.0, "%s: err/E = %.3f" % (what, worst)
    return worst


def box_signed_distance(points, half=0.5):
    """The analytic signed distance to the axis-aligned cube [-half, half]^3 in float64: negative inside."""
    q = points.double().abs() - half
    outside = q.clamp(min=0).norm(dim=-1)
    inside = q.max(dim=-1).values.clamp(max=0)
    return outside + inside
