"""Float64 restatement of mesh_renderer.points.cast_rays, written from the definition (include/mesh_raster.h;
INTEGRATION.md, "Point-cloud losses"), its a-posteriori rounding bounds, and the inputs the host and the GPU tests share.

Per ray: kz = the first axis that attains max |d_k|, kx = (kz + 1) % 3, ky = (kz + 2) % 3, exchanged when d[kz] < 0,
S = (d[kx], d[ky], 1) / d[kz].  Per corner p = v - o: Px = fma(-Sx, p[kz], p[kx]), Py likewise, Pz = Sz p[kz].
U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax; reject on mixed signs and on det = U + V + W == 0;
t = (U Az + V Bz + W Cz) / det, accepted in [t_min, t_max]; bary = (U, V, W) / det; the least t wins, the lowest face
of equal t.  evaluate() is that text on the float32 inputs promoted to float64 (and, for the calibration only, in
float32 operation by operation).

THE BOUNDS, with eps = 2^-24 and one constant C.  A sheared coordinate carries the rounding of p, of S and of its own
fused multiply-add, each relative to m_x(P) = |p[kx]| + |Sx p[kz]| (m_y alike), so an edge function is off by at most
  E_U = C eps [ (|Cx By| + |Cy Bx|)  +  (m_x(C) |By| + |Cx| m_y(B) + m_y(C) |Bx| + |Cy| m_x(B)) ]
-- its own two products and difference, plus what Ax .. Cy carried in -- and from there, by the same first-order rules,
  E_det = E_U + E_V + E_W + C eps |det|
  E_T   = E_U |Az| + E_V |Bz| + E_W |Cz| + C eps (|U Az| + |V Bz| + |W Cz|)
  E_t   = (E_T + |t| E_det) / |det| + eps |t|
  E_bary(U) = (E_U + |U / det| E_det) / |det| + eps.
CALIBRATION (python tests/ray_reference.py, on the CPU): in units of the bounds at C = 1 the float32 evaluation of the
definition -- the arithmetic of the package's float32 torch route, operation by operation -- reaches err/E = 1.20 on an
edge function (soup_5), 0.38 on t (soup_translated) and 0.84 on a barycentric (soup_7) over every case below.  C = 6
therefore holds the torch route at or below 0.20 and leaves the HIP kernels, whose operations are the same IEEE
operations, a factor of 5.

WHICH RAYS ARE DECIDED.  A pair is decided when |U| > E_U, |V| > E_V and |W| > E_W and, unless its signs are mixed, t
is further than E_t from t_min and from t_max.  A decided pair is certainly accepted or certainly rejected in float32.
A ray is decided when some pair is certainly accepted and the certainly accepted pair w with the least t is clear of
every other pair j that is not certainly rejected -- decided or not --: t_j - E_t(j) > t_w + E_t(w) (an exact copy of
w's index triple is exempt: it computes the same bits, and the lower face wins in both precisions); or when every pair
is certainly rejected (a miss).  A decided ray must name the restatement's face with |t - t64| <= E_t and every
barycentric within E_bary; an undecided ray must be a miss or name a face whose float64 evaluation does not certainly
reject it, with t within E_t of that face's.  So that the bounds cannot hide a failure, in every case at least
DECIDED_SHARE of the valid rays are decided and at least EASY_SHARE of the decided hits have E_t <= 1e-3 max(1, t);
check() asserts both, and the host test asserts them on the restatement alone.

THE GRADIENT BOUND.  With n = (b - a) x (c - a), s = n . d, g = n / s and M = |b - a| |c - a|, a float32 n is off by a
few eps M and s by a few eps M |d|, so  E_g = C_G eps (M / |s|) (1 + |n| |d| / |s|)  bounds every component of g.  For
the weighted sum L = sum_i w_i t_i, faces, t and barycentrics taken from the result under test:
  E(dL/do_i) = |w_i| (E_g + eps |g|),    E(dL/dd_i) = |w_i| (t E_g + E_t |g| + 2 eps t |g|),
  E(dL/dv)   = sum over the (ray, corner) entries naming v of |w_i| (|bary| E_g + E_bary |g|) + (2 + count) eps |w_i bary| |g|
(the last term: the products and the fixed-order sum of `count` entries).  Calibrated like C: in units of the bound at
C_G = 1 the float32 torch route's analytic gradients reach 1.03 (sphere); C_G = 5 holds them at or below 0.21 and leaves
the kernels, which contract their products, a factor of 5.
"""
import math

import numpy as np
import torch

import point_mesh_reference as pm
import winding_reference as wr
from pytorch_mesh_renderer_amd.common import shapes

INF = float("inf")
EPS = 2.0 ** -24
C = 6.0                 # measured need: 1.20 (see above)
C_G = 5.0               # measured need: 1.03
DECIDED_SHARE = 0.95
EASY_SHARE = 0.9
EASY_BOUND = 1e-3
OFFSET = wr.OFFSET
NAMES = ["soup_%s" % k for k in wr.SOUPS] + ["cube", "sphere", "cube_translated", "sphere_translated"]

_cases = {}
_truth = {}


def _rays(rng, B, N, offset=None):
    """Origins on the sphere of radius 3 around the meshes' cube [-1, 1]^3, aimed at random points inside it; the
    directions are not normalised."""
    start = rng.normal(size=(B, N, 3))
    start = 3.0 * start / np.linalg.norm(start, axis=-1, keepdims=True)
    aim = rng.uniform(-1, 1, (B, N, 3))
    direction = (aim - start) * rng.uniform(0.5, 2.0, (B, N, 1))
    if offset is not None:
        start = start + np.asarray(offset)
    return torch.from_numpy(start.astype(np.float32)), torch.from_numpy(direction.astype(np.float32))


def _shape_case(name):
    base = name.split("_")[0]
    offset = OFFSET if name.endswith("_translated") else None
    if base == "cube":
        v, t, _ = shapes.cube(1.0)
        v, t, B, N = v.double().numpy()[None].repeat(2, 0), t.long(), 2, 300
    else:
        v, t, _ = shapes.sphere_arrays(1.0, 25)
        v, t, B, N = v.astype(np.float64)[None], torch.from_numpy(t.astype(np.int64)), 1, 700
    o, d = _rays(np.random.default_rng(len(name) + 700), B, N, offset)
    if offset is not None:
        v = v + np.asarray(offset)
    return o, d, torch.from_numpy(v.astype(np.float32)), t


def case(name):
    """-> (origins [B,N,3] f32, directions [B,N,3] f32, vertices [B,V,3] f32, triangles [T,3] i64), built once."""
    if name not in _cases:
        if name.startswith("soup_"):
            k = name[5:]
            p, v, t = pm.mesh(k if k == "translated" else int(k))
            o, d = _rays(np.random.default_rng(900 + len(_cases)), p.shape[0], p.shape[1], OFFSET if k == "translated" else None)
            _cases[name] = (o, d, v, t)
        else:
            _cases[name] = _shape_case(name)
    return _cases[name]


def closed_mesh():
    """An octahedron subdivided twice onto the unit sphere (66 vertices, 128 triangles, every edge shared by exactly
    two of them), rotated by an arbitrary rotation and moved by OFFSET -> (vertices [66,3] f32, triangles [128,3] i64,
    an interior point [3] f32)."""
    verts = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    verts = [np.asarray(x, dtype=np.float64) for x in verts]
    tris = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(2):
        middle, out = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in middle:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                middle[key] = len(verts) - 1
            return middle[key]

        for a, b, c in tris:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        tris = out
    axis = np.asarray([0.3, -0.5, 0.8])
    axis = axis / np.linalg.norm(axis)
    angle = 0.7123
    K = np.asarray([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K
    v = np.stack(verts) @ R.T + np.asarray(OFFSET)
    inside = np.asarray(OFFSET) + np.asarray([0.11, -0.07, 0.05])
    return (torch.from_numpy(v.astype(np.float32)), torch.tensor(tris, dtype=torch.int64),
            torch.from_numpy(inside.astype(np.float32)))


def watertight_rays(vertices, triangles, inside, count=2000, seed=77):
    """Rays from `inside` [3] at every vertex, at five float32 points on every edge and in `count` random directions
    -> (origins [N,3] f32, directions [N,3] f32)."""
    t = triangles.long()
    edges = torch.cat([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]).sort(dim=1).values.unique(dim=0)
    a, b = vertices[edges[:, 0]], vertices[edges[:, 1]]
    on_edges = torch.cat([a + s * (b - a) for s in (0.1, 0.3, 0.5, 0.7, 0.9)])
    g = torch.Generator().manual_seed(seed)
    aims = torch.cat([vertices - inside, on_edges - inside, torch.randn(count, 3, generator=g)])
    return inside[None].expand(aims.shape[0], 3).contiguous(), aims.contiguous()


def usable(vertices, triangles):
    """[B,T]: every index in [0, V), no two equal, every corner finite."""
    v, t = vertices, triangles.long()
    V = v.shape[1]
    ok = ((t >= 0) & (t < V)).all(dim=1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])
    safe = t.clamp(0, V - 1)
    finite = torch.isfinite(v).all(-1)
    return ok[None] & finite[:, safe[:, 0]] & finite[:, safe[:, 1]] & finite[:, safe[:, 2]]


def _pick(x, k):
    return torch.gather(x, -1, k[..., None].expand(*x.shape[:-1], 1))[..., 0]


class Pairs:
    """Everything evaluate() knows of every (ray, triangle) pair, [B,N,T] each, and of every ray, [B,N]."""


def evaluate(origins, directions, vertices, triangles, lengths=None, t_min=0.0, t_max=INF, dtype=torch.float64):
    """The definition on every pair in `dtype` (float64: the restatement; float32: the calibration's float32 twin,
    with the fused multiply-add formed in float64, where its product is exact, and the exact-zero recomputation) with
    the bounds of the docstring above -> Pairs."""
    o, d, v = origins.to(dtype), directions.to(dtype), vertices.to(dtype)
    tri = triangles.long()
    B, N = o.shape[:2]
    V = v.shape[1]
    safe = tri.clamp(0, V - 1)
    size = d.abs().max(-1).values
    live = (torch.isfinite(o).all(-1) & torch.isfinite(d).all(-1) & (size > 0)
            & (torch.arange(N)[None, :] < pm._valid(lengths, B, N)[:, None]))
    o = torch.where(live[..., None], o, torch.zeros_like(o))
    d = torch.where(live[..., None], d, torch.ones_like(d))
    kz = torch.from_numpy(np.argmax((d.abs() == d.abs().max(-1, keepdim=True).values).numpy(), axis=-1))   # the first
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    dz = _pick(d, kz)
    kx, ky = torch.where(dz < 0, ky, kx), torch.where(dz < 0, kx, ky)
    sx, sy, sz = _pick(d, kx) / dz, _pick(d, ky) / dz, 1.0 / dz
    p = v[:, None] - o[:, :, None]                                                        # [B,N,V,3]
    along = lambda k: _pick(p, k[..., None].expand(B, N, V))
    pk, pkx, pky = along(kz), along(kx), along(ky)
    fma = lambda a, b, c: (a.double() * b.double() + c.double()).to(dtype)
    px, py, pz = fma(-sx[..., None], pk, pkx), fma(-sy[..., None], pk, pky), sz[..., None] * pk
    mx, my = pkx.abs() + (sx[..., None] * pk).abs(), pky.abs() + (sy[..., None] * pk).abs()
    corner = lambda x: [x[:, :, safe[:, k]] for k in range(3)]                            # [B,N,T] x 3
    (ax, bx, cx), (ay, by, cy), (az, bz, cz) = corner(px), corner(py), corner(pz)
    (max_, mbx, mcx), (may, mby, mcy) = corner(mx), corner(my)

    def edge(x1, y2, y1, x2):   # x1 y2 - y1 x2
        value = x1 * y2 - y1 * x2
        return value, (x1 * y2).abs() + (y1 * x2).abs()

    q = Pairs()
    q.U, mu = edge(cx, by, cy, bx)
    q.V, mv = edge(ax, cy, ay, cx)
    q.W, mw = edge(bx, ay, by, ax)
    if dtype != torch.float64:
        zero = (q.U == 0) | (q.V == 0) | (q.W == 0)
        wide = [x.double() for x in (ax, ay, bx, by, cx, cy)]
        ax_, ay_, bx_, by_, cx_, cy_ = wide
        q.sign = [torch.where(zero, a_, b_.double()) for a_, b_ in
                  ((cx_ * by_ - cy_ * bx_, q.U), (ax_ * cy_ - ay_ * cx_, q.V), (bx_ * ay_ - by_ * ax_, q.W))]
        q.U, q.V, q.W = (x.to(dtype) for x in q.sign)
    else:
        q.sign = [q.U, q.V, q.W]
    q.EU = C * EPS * (mu + mcx * by.abs() + cx.abs() * mby + mcy * bx.abs() + cy.abs() * mbx)
    q.EV = C * EPS * (mv + max_ * cy.abs() + ax.abs() * mcy + may * cx.abs() + ay.abs() * mcx)
    q.EW = C * EPS * (mw + mbx * ay.abs() + bx.abs() * may + mby * ax.abs() + by.abs() * max_)
    q.det = (q.U + q.V) + q.W
    top = (q.U * az + q.V * bz) + q.W * cz
    q.t = top / q.det
    adet = q.det.abs()
    q.Edet = q.EU + q.EV + q.EW + C * EPS * adet
    ET = (q.EU * az.abs() + q.EV * bz.abs() + q.EW * cz.abs()
          + C * EPS * ((q.U * az).abs() + (q.V * bz).abs() + (q.W * cz).abs()))
    q.Et = (ET + q.t.abs() * q.Edet) / adet + EPS * q.t.abs()
    q.bary = torch.stack([q.U, q.V, q.W], -1) / q.det[..., None]
    q.Ebary = (torch.stack([q.EU, q.EV, q.EW], -1) + q.bary.abs() * q.Edet[..., None]) / adet[..., None] + EPS
    s0, s1, s2 = q.sign
    q.mixed = ((s0 < 0) | (s1 < 0) | (s2 < 0)) & ((s0 > 0) | (s1 > 0) | (s2 > 0))
    q.usable = usable(v, tri)[:, None, :] & live[..., None]
    q.live = live
    q.accept = q.usable & ~q.mixed & (q.det != 0) & (q.t >= t_min) & (q.t <= t_max)
    q.t_min, q.t_max = t_min, t_max
    return q


def first_hit(q):
    """The definition's answer on evaluate()'s pairs -> (t [B,N] (+inf for a miss), face [B,N] i64 (-1), bary [B,N,3])."""
    t = torch.where(q.accept, torch.where(q.t == 0, torch.zeros_like(q.t), q.t), torch.full_like(q.t, INF))
    face = torch.from_numpy(np.argmin(t.numpy(), axis=2))                                 # numpy: the first of equal minima
    best = torch.gather(t, 2, face[..., None])[..., 0]
    hit = best < INF
    bary = torch.gather(q.bary, 2, face[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
    return best, torch.where(hit, face, torch.full_like(face, -1)), torch.where(hit[..., None], bary, torch.zeros_like(bary))


class Truth:
    """The restatement of one case: the pairs q, the first hit (t, face, bary), which rays are decided, and the bounds
    at the winning face (Et [B,N], Ebary [B,N,3])."""


def truth_of(origins, directions, vertices, triangles, lengths=None, t_min=0.0, t_max=INF):
    q = evaluate(origins, directions, vertices, triangles, lengths, t_min, t_max)
    r = Truth()
    r.q, r.triangles = q, triangles.long()
    r.t, r.face, r.bary = first_hit(q)
    sure = (q.U.abs() > q.EU) & (q.V.abs() > q.EV) & (q.W.abs() > q.EW)
    below, above = q.t < t_min - q.Et, q.t > t_max + q.Et
    inside = (q.t > t_min + q.Et) & (q.t < t_max - q.Et if t_max < INF else torch.isfinite(q.t))
    r.rejected = ~q.usable | (sure & (q.mixed | below | above))                           # certainly
    r.accepted = q.usable & sure & ~q.mixed & inside                                      # certainly
    sure_t = torch.where(r.accepted, q.t, torch.full_like(q.t, INF))
    w = torch.from_numpy(np.argmin(sure_t.numpy(), axis=2))
    have = torch.gather(sure_t, 2, w[..., None])[..., 0] < INF
    at = lambda x: torch.gather(x, 2, w[..., None])[..., 0]
    reach = at(q.t) + at(q.Et)                                                            # t_w + E_t(w)
    near = torch.where(torch.isfinite(q.t) & torch.isfinite(q.Et), q.t - q.Et, torch.full_like(q.t, -INF))
    copy = (r.triangles[None, None, :, :] == r.triangles[w][:, :, None, :]).all(-1)                      # [B,N,T]: w itself and its copies
    clear = r.rejected | copy | (near > reach[..., None])
    miss = r.rejected.all(-1)
    r.decided = q.live & ((have & clear.all(-1)) | miss) | ~q.live
    # a decided ray's winner is the definition's first hit
    assert bool(((r.face == torch.where(have, w, torch.full_like(w, -1))) | ~r.decided | ~q.live).all())
    pick = r.face.clamp(min=0)
    r.Et = torch.where(r.face >= 0, torch.gather(q.Et, 2, pick[..., None])[..., 0], torch.zeros_like(r.t))
    r.Ebary = torch.gather(q.Ebary, 2, pick[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
    r.valid = torch.arange(r.t.shape[1])[None, :] < pm._valid(lengths, *r.t.shape)[:, None]
    return r


def truth(name):
    """truth_of(*case(name)), computed once and shared."""
    if name not in _truth:
        _truth[name] = truth_of(*case(name))
    return _truth[name]


def shares(r):
    """-> (the share of the valid rays that are decided, the share of the decided hits with E_t <= 1e-3 max(1, t))."""
    decided = float(r.decided[r.valid].double().mean()) if bool(r.valid.any()) else 1.0
    hits = r.decided & r.valid & (r.face >= 0)
    easy = float((r.Et[hits] <= EASY_BOUND * r.t[hits].clamp(min=1.0)).double().mean()) if bool(hits.any()) else 1.0
    return decided, easy


def check(t, face, bary, r, what, demand_shares=True):
    """A result against the restatement under the rules of the docstring above; the figures are printed first.
    -> the worst err/E of t and of the barycentrics over the decided hits."""
    t, face, bary = t.detach().double().cpu(), face.cpu().long(), bary.detach().double().cpu()
    q = r.q
    assert t.shape == r.t.shape and face.shape == r.face.shape and bary.shape == r.bary.shape
    assert not bool(torch.isnan(t).any()) and not bool(torch.isnan(bary).any()), "%s: NaN in a result" % what
    miss = face < 0
    assert bool((face[miss] == -1).all()) and bool((t[miss] == INF).all()) and bool((bary[miss] == 0).all()), what
    assert bool((face < q.t.shape[2]).all()) and bool(torch.isfinite(t[~miss]).all()) and bool((t[~miss] >= 0).all()), what
    assert bool(miss[~q.live].all()), "%s: a dead or padded ray has a hit" % what
    decided, easy = shares(r)
    hits = r.decided & (r.face >= 0)
    same = face == r.face
    ratio_t = ((t - r.t).abs() / r.Et)[hits & same]
    ratio_b = ((bary - r.bary).abs() / r.Ebary)[hits & same]
    worst_t = float(ratio_t.max()) if ratio_t.numel() else 0.0
    worst_b = float(ratio_b.max()) if ratio_b.numel() else 0.0
    # an undecided ray: a miss, or a face the float64 evaluation does not certainly reject, with that face's t
    loose = ~r.decided & ~miss
    pick = face.clamp(min=0)[..., None]
    t_at, e_at = torch.gather(q.t, 2, pick)[..., 0], torch.gather(q.Et, 2, pick)[..., 0]
    tolerable = ~torch.gather(r.rejected, 2, pick)[..., 0] & ((t - t_at).abs() <= e_at)
    print("%s: %d rays, %d hits, decided %.4f, easy %.4f, worst err/E t %.3f bary %.3f, undecided hits %d"
          % (what, int(r.valid.sum()), int((r.face >= 0).sum()), decided, easy, worst_t, worst_b, int(loose.sum())))
    if demand_shares:
        assert decided >= DECIDED_SHARE, "%s: only %.3f of the rays are decided" % (what, decided)
        assert easy >= EASY_SHARE, "%s: the bound is loose on %.3f of the decided hits" % (what, 1 - easy)
    assert bool(same[r.decided].all()), "%s: %d decided rays name another face" % (what, int((~same & r.decided).sum()))
    assert worst_t <= 1.0, "%s: t err/E = %.3f" % (what, worst_t)
    assert worst_b <= 1.0, "%s: bary err/E = %.3f" % (what, worst_b)
    assert bool(tolerable[loose].all()), "%s: an undecided ray names a face float64 rejects" % what
    return max(worst_t, worst_b)


def check_watertight(cast):
    """Every ray from an interior point at every vertex, at five points on every edge and in 2000 random directions
    hits, on the cube (from its centre, where the edge functions are exactly 0, and from an arbitrary point) and on the
    rotated, translated closed mesh of the reference file."""
    v, tri, _ = shapes.cube(1.0)
    closed_v, closed_tri, inside = closed_mesh()
    for what, vertices, triangles, start in (("cube from its centre", v, tri.long(), torch.zeros(3)),
                                             ("cube", v, tri.long(), torch.tensor([0.11, -0.07, 0.05])),
                                             ("closed mesh", closed_v, closed_tri, inside)):
        o, d = watertight_rays(vertices, triangles, start)
        t, face, bary = cast(o, d, vertices, triangles)
        missed = int((face < 0).sum())
        print("%s: %d rays, %d missed" % (what, o.shape[0], missed))
        assert o.shape[0] == vertices.shape[0] + 5 * (3 * triangles.shape[0] // 2) + 2000
        assert missed == 0, "%s: %d rays slip through" % (what, missed)
        assert bool(torch.isfinite(t).all()) and bool((t > 0).all())
        r = truth_of(o[None], d[None], vertices[None], triangles)
        check(t[None], face[None], bary[None], r, what, demand_shares=False)



# ---- gradients ------------------------------------------------------------------------------------------------------------

def _corners(vertices, triangles, face):
    tri = triangles.long().clamp(0, vertices.shape[1] - 1)[face.long().clamp(min=0)]      # [B,N,3]
    return tri, [torch.gather(vertices, 1, tri[..., k, None].expand(-1, -1, 3)) for k in range(3)]


def gradients(origins, directions, vertices, triangles, face, weights):
    """float64 autograd of sum_i w_i t_i with t = n . (a - o) / (n . d), n = (b - a) x (c - a), at the GIVEN faces
    (-1: no term; a ray with n . d == 0 has no term either) -> (dorigins, ddirections, dvertices)."""
    o, d, v = (x.detach().double().clone().requires_grad_(True) for x in (origins, directions, vertices))
    _, (a, b, c) = _corners(v, triangles, face)
    n = torch.cross(b - a, c - a, dim=-1)
    s = (n * d).sum(-1)
    have = (face.long() >= 0) & (s != 0)
    t = (n * (a - o)).sum(-1) / torch.where(have, s, torch.ones_like(s))
    (torch.where(have, t, torch.zeros_like(t)) * weights.double()).sum().backward()
    return o.grad, d.grad, v.grad


def gradient_bounds(origins, directions, vertices, triangles, t, face, bary, weights, q):
    """The bounds of the docstring above for a result (t, face, bary) and the pairs q of its case ->
    (E_dorigins [B,N,1], E_ddirections [B,N,1], E_dvertices [B,V,1]); +inf where n . d == 0."""
    o, d, v = origins.double(), directions.double(), vertices.double()
    t, bary, w = t.detach().double().cpu(), bary.detach().double().cpu(), weights.double().cpu().abs()
    face = face.cpu().long()
    tri, (a, b, c) = _corners(v, triangles, face)
    n = torch.cross(b - a, c - a, dim=-1)
    s = (n * d).sum(-1).abs()
    hit = face >= 0
    s = torch.where(hit, s, torch.ones_like(s))
    M = (b - a).norm(dim=-1) * (c - a).norm(dim=-1)
    g = n.norm(dim=-1) / s
    Eg = C_G * EPS * (M / s) * (1 + n.norm(dim=-1) * d.norm(dim=-1) / s)
    pick = face.clamp(min=0)
    Et = torch.gather(q.Et, 2, pick[..., None])[..., 0]
    Eb = torch.gather(q.Ebary, 2, pick[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]    # [B,N,3]
    tt = torch.where(hit, t, torch.zeros_like(t))
    zero = torch.zeros_like(s)
    Eo = torch.where(hit, w * (Eg + EPS * g), zero)
    Ed = torch.where(hit, w * (tt * Eg + Et * g + 2 * EPS * tt * g), zero)
    per = w[..., None] * (bary.abs() * Eg[..., None] + Eb * g[..., None])                  # [B,N,3]
    mag = w[..., None] * bary.abs() * g[..., None]
    per, mag = (torch.where(hit[..., None], x, torch.zeros_like(x)) for x in (per, mag))
    B, V = v.shape[:2]
    Ev, total, count = (torch.zeros(B, V, dtype=torch.float64) for _ in range(3))
    for k in range(3):
        Ev.scatter_add_(1, tri[..., k], per[..., k])
        total.scatter_add_(1, tri[..., k], mag[..., k])
        count.scatter_add_(1, tri[..., k], hit.double())
    Ev = Ev + (2 + count) * EPS * total
    return Eo[..., None], Ed[..., None], Ev[..., None]


def check_gradients(got, want, bounds, what):
    """Each of (dorigins, ddirections, dvertices) within its bound component by component -> the worst err/E."""
    worst = 0.0
    for name, x, y, e in zip(("dorigins", "ddirections", "dvertices"), got, want, bounds):
        x = x.detach().double().cpu()
        assert bool(torch.isfinite(x).all()), "%s %s: not finite" % (what, name)
        err = (x - y).abs()
        e = e.expand_as(err)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / e)
        finite = torch.isfinite(e)
        share = float((e[finite] <= 1e-3 * y.abs().max().clamp(min=1e-30)).double().mean())
        print("%s %s: worst err/E %.3f, max err %.3g of scale %.3g, share of bounds <= 1e-3 scale %.3f"
              % (what, name, float(ratio.max()), float(err[finite].max()), float(y.abs().max()), share))
        assert share >= EASY_SHARE, "%s %s: the bound is loose" % (what, name)
        assert float(ratio.max()) <= 1.0, "%s %s: err/E = %.3f" % (what, name, float(ratio.max()))
        worst = max(worst, float(ratio.max()))
    return worst


def _calibrate():
    """The figures of the docstring: the float32 twin of the definition, and the float32 torch route's gradients,
    against float64 in units of the bounds at C = C_G = 1."""
    from pytorch_mesh_renderer_amd import mesh_renderer
    worst = {"edge": 0.0, "t": 0.0, "bary": 0.0, "grad": 0.0}
    for name in NAMES:
        o, d, v, tri = case(name)
        r = truth(name)
        q, f = r.q, evaluate(o, d, v, tri, dtype=torch.float32)
        keep = q.usable
        edge = max(float(((a.double() - b).abs() / e)[keep].max()) for a, b, e in
                   ((f.U, q.U, q.EU), (f.V, q.V, q.EV), (f.W, q.W, q.EW))) * C if bool(keep.any()) else 0.0
        sure = r.accepted
        tt = float(((f.t.double() - q.t).abs() / q.Et)[sure].max()) * C if bool(sure.any()) else 0.0
        bb = float(((f.bary.double() - q.bary).abs() / q.Ebary)[sure].max()) * C if bool(sure.any()) else 0.0
        og, dg, vg = (x.clone().requires_grad_(True) for x in (o, d, v))
        t, face, bary = mesh_renderer.points.cast_rays(og, dg, vg, tri)
        w = torch.randn(t.shape, generator=torch.Generator().manual_seed(3))
        torch.where(face >= 0, t, torch.zeros_like(t)).mul(w).sum().backward()
        want = gradients(o, d, v, tri, face, w)
        bounds = gradient_bounds(o, d, v, tri, t, face, bary, w, q)
        gg = 0.0
        for x, y, e in zip((og.grad, dg.grad, vg.grad), want, bounds):
            err = (x.double() - y).abs()
            ratio = torch.where(err == 0, torch.zeros_like(err), err / e.expand_as(err))
            gg = max(gg, float(ratio.max()) * C_G)
        print("%-18s %s edge %.3f t %.3f bary %.3f grad %.3f (in units of the bounds at C = C_G = 1)"
              % (name, "decided %.4f easy %.4f" % shares(r), edge, tt, bb, gg))
        for k, x in zip(("edge", "t", "bary", "grad"), (edge, tt, bb, gg)):
            worst[k] = max(worst[k], x)
    print("worst:", worst)


if __name__ == "__main__":
    _calibrate()
