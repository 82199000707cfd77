"""Float64 truth of the mesh regularisers with a-posteriori float32 rounding bounds, a float32 restatement of the
stable formulas, and the cases the host and the GPU truth tests share (test_regularizers_truth_host.py / _gpu.py).

The topology is mesh_regularizer_reference.topology (plain loops, nothing of the package); the terms are evaluated
over it with index_add in float64, so a mesh of 8k vertices costs a second.  u = 2^-24 throughout.

VALUES, per image (the float32 inputs are exact, every bound is computed in float64 from them alone):
  lap   delta_i = (1/deg_i) sum_j (v_j - v_i).  Each difference is one rounding, u |v_j - v_i|, and the sum and the
        product with 1/deg add a few more of the same size, so |err(delta_i)| <= k u r_i with
        r_i = (1/deg_i) sum_j |v_j - v_i|, and | |delta_i| - its float32 | <= the same:
            E_lap = K_LAP u (1/V) sum_i r_i.
        Only neighbour distances enter: the bound does not grow when the mesh is translated, so a kernel that forms
        (1/deg) sum v_j - v_i and cancels against |v| fails it.
  edge  len = |v_lo - v_hi| is a rounded difference, three products, two sums and a root: (a few) u len.
            E_edge = K_EDGE u (1/E) sum len                                      without a target,
            E_edge = K_EDGE u (1/E) sum (2 len |len - t| + (len - t)^2)          with the target t:
        d(len - t)^2 = 2 |len - t| err(len), and the square itself rounds by u (len - t)^2.
  nc    per flap, p = b - a, q = c - a, r = d - a, n0 = p x q, n1 = r x p, h = n / |n|.  Every component of a cross
        product is a difference of two products of magnitude <= |p||q|, so the DIRECTION of n0 is off by up to
        u |p||q| / |n0| = u kappa0 (kappa0 = 1 / sin of the angle at a: large for slivers), likewise kappa1 =
        |r||p| / |n1|.  With delta_f = u (kappa0 + kappa1) the computed h0 - h1 is off by a vector e, |e| <= k delta_f,
        and |h0 - h1|^2 / 2 moves by (h0 - h1).e + |e|^2 / 2; the lengths |h| = 1 +- 2u scale the value by 1 +- 4u:
            E_f = K_NC (delta_f |h0 - h1| + delta_f^2) + 4 u (1 - cos),      E_nc = (1/F) sum_f E_f.
        A formulation that subtracts cos from 1 carries u per flap whatever the angle and fails this bound once
        |h0 - h1| = theta is small.  A flap at or below the 1e-8 floor has value 0 and E_f = 0.

GRADIENT, per vertex and with no vertex exempt: |got_v - want_v| (Euclidean) <= E_v = u (K_GRAD_LAP A_lap +
K_GRAD_EDGE A_edge + K_GRAD_NC A_nc), each A the float64 sum of the magnitudes of the entries the backward gathers
into v, each magnitude carrying the conditioning of the entry (g = dterms of the image):
  lap   dL/dv_k = (g0 / V) (-u_k + sum_{i in N(k)} u_i / deg_i), u_i = delta_i / |delta_i|.  u_i is a direction: the
        error k u r_i of delta_i turns it by up to k u r_i / |delta_i|, and normalising adds (a few) u.  So the entry
        u_i counts with w_i = 1 + r_i / |delta_i| (0 where delta_i = 0):
            A_lap(k) = |g0| / V (w_k + sum_{i in N(k)} w_i / deg_i).
        On a smooth regular mesh |delta_i| << r_i and the direction is ill-conditioned in ANY float32 formulation;
        w_i says by how much, from the geometry alone.
  edge  d len / dv = (v - v_j) / len, a rounded difference over its own rounded length: magnitude 1, error (a few) u.
        With a target the factor 2 (len - t) carries err(len) = u len next to its own size:
            A_edge(k) = |g1| / E sum_{edges at k} 1      or      |g1| / E sum_{edges at k} 2 (|len - t| + len).
  nc    C = h0 . h1.  dC/dn0 = (h1 - C h0) / |n0| = g0, dC/dn1 = (h0 - C h1) / |n1| = g1, |h1 - C h0| = |h0 - C h1| =
        sin(theta).  g0 is orthogonal to h0 and (as h0 and h1 both are) to p, so |g0 x p| = |g0| |p|:
            dC/dc = g0 x p                  lever |p| / |n0|
            dC/dd = p x g1                  lever |p| / |n1|
            dC/db = q x g0 + g1 x r         lever |q| / |n0| + |r| / |n1|
            dC/da = -(the three) = -((q - p) x g0 + g1 x (r - p))      lever |c - b| / |n0| + |d - b| / |n1|
        and |dC/d vertex| <= sin(theta) lever.  The computed h1 - C h0 is off by the direction errors of both
        normals, delta_f / u = kappa0 + kappa1, whatever theta is: the inherent 1/theta floor of float32 normals.
        So the entry counts with (sin(theta) + kappa0 + kappa1) lever:
            A_nc(k) = |g2| / F sum_{(flap, role) at k} (sin(theta) + kappa0 + kappa1) lever(role).

THE CONSTANTS are powers of two, each the smallest that keeps the float32 torch evaluation of the stable formulas
(restatement32 below: the difference-form Laplacian and |h0 - h1|^2 / 2, autograd gradients, on the CPU; never the
kernel, never the package's torch path) at or below 1/4 of the bound on every case of CASES, every term also run
alone; the kernels get the remaining factor of 4 for their summation orders, fused multiply-adds and 1-ulp roots.
Chosen: K_LAP 8, K_EDGE 16, K_NC 1/2, K_GRAD_LAP 4, K_GRAD_EDGE 16, K_GRAD_NC 4; the measured ratios are in
test_regularizers_truth_host.py (restatement) and test_regularizers_truth_gpu.py (kernels).

THE CAP, so that a bound cannot grow until it hides a failure (check() asserts it and prints the share): in every run
at least 90 % of the vertices have E_v <= 1e-4 max|expected gradient| -- the budget of test_regularizers_gpu.py, so on
those vertices the check is nowhere looser than that one -- and every value bound is <= 1e-5 |value|.  This is a
condition on the cases, not a measurement: a case whose shape is free is shaped to meet it (the sliver is grid_1e-1
squeezed, not a flatter grid).  The grids at sigma = 1e-2, 1e-3 and 1e-4 and the planar grid are named cases that
cannot meet it in some runs; CAPS lists those runs, each with the first decade that holds and the reason.
"""
import collections
import itertools

import torch

import mesh_regularizer_reference as ref

U = 2.0 ** -24
K_LAP = 8.0
K_EDGE = 16.0
K_NC = 0.5
K_GRAD_LAP = 4.0
K_GRAD_EDGE = 16.0
K_GRAD_NC = 4.0
NORMAL_FLOOR = 1e-8
OFFSET = (100.0, -50.0, 25.0)
OFFSETS = {"0": (0.0, 0.0, 0.0), "10": (10.0, -5.0, 2.5), "100": OFFSET, "1000": (1000.0, -500.0, 250.0)}
EASY_GRADIENT = 1e-4
EASY_SHARE = 0.9
VERTICES_PER_BLOCK, FLAPS_PER_BLOCK, ROWS_PER_TRIP = 32, 256, 256    # csrc/mesh_reg.hip's launch shape

Truth = collections.namedtuple("Truth", "values grad e_values e_grad")
Case = collections.namedtuple("Case", "vertices triangles topo dterms runs")


def index(topo):
    """The loop-built topology as index tensors (cached in the dict): edges [E,2], flaps [F,4], the directed edges
    src -> dst [2E] and the degrees [V] float64."""
    if "_index" not in topo:
        e = torch.tensor(topo["edges"], dtype=torch.long).reshape(-1, 2)
        f = torch.tensor(topo["flaps"], dtype=torch.long).reshape(-1, 4)
        src, dst = torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])
        deg = torch.zeros(topo["V"], dtype=torch.float64).index_add_(0, src, torch.ones(src.shape[0], dtype=torch.float64))
        topo["_index"] = (e, f, src, dst, deg)
    return topo["_index"]


def _norm(x):
    return ref._norm(x)


def _gather(B, V, where, entries):
    """sum the entries [B,n] into the vertices `where` [n] -> [B,V]"""
    return torch.zeros(B, V, dtype=entries.dtype).index_add_(1, where, entries)


def _evaluate(v, topo, laplacian, edge, normal, target_length, lap_form="difference", nc_form="half"):
    """The three terms [B,3] in the dtype of v over the loop-built topology, and what the bounds need of them."""
    e, f, src, dst, deg = index(topo)
    B, V = v.shape[0], v.shape[1]
    zero = v.new_zeros(B)
    lap, edg, nc = zero, zero, zero
    parts = {}
    safe_deg = deg.clamp(min=1).to(v.dtype)[None, :, None]
    if laplacian and e.shape[0] > 0:
        if lap_form == "difference":
            diff = v[:, dst] - v[:, src]
            delta = torch.zeros_like(v).index_add(1, src, diff) / safe_deg
        else:   # the sum-then-subtract form the kernel had: what the bound must refuse
            sums = torch.zeros_like(v).index_add(1, src, v[:, dst])
            delta = torch.where((deg > 0)[None, :, None], sums / safe_deg - v, torch.zeros_like(v))
        length = _norm(delta)
        lap = length.sum(1) / V
        parts["delta_len"] = length
    if edge and e.shape[0] > 0:
        length = _norm(v[:, e[:, 0]] - v[:, e[:, 1]])
        edg = (length if target_length is None else (length - float(target_length)) ** 2).sum(1) / e.shape[0]
        parts["edge_len"] = length
    if normal and f.shape[0] > 0:
        a, b, c, d = (v[:, f[:, k]] for k in range(4))
        p, q, r = b - a, c - a, d - a
        n0, n1 = torch.cross(p, q, dim=-1), torch.cross(r, p, dim=-1)
        l0, l1 = _norm(n0), _norm(n1)
        ok = (l0 > NORMAL_FLOOR) & (l1 > NORMAL_FLOOR)
        one = torch.ones_like(l0)
        s0, s1 = torch.where(ok, l0, one), torch.where(ok, l1, one)
        if nc_form == "half":
            w = n0 / s0[..., None] - n1 / s1[..., None]
            per = 0.5 * (w * w).sum(-1)
        else:   # 1 - cos, as the kernel had it
            per = 1.0 - (n0 * n1).sum(-1) / (s0 * s1)
        nc = torch.where(ok, per, torch.zeros_like(per)).sum(1) / f.shape[0]
        parts.update(ok=ok, p=p, q=q, r=r, cb=c - b, db=d - b, l0=s0, l1=s1, h0=n0 / s0[..., None],
                     h1=n1 / s1[..., None], per=per)
    return torch.stack([lap, edg, nc], dim=1), parts


def truth(vertices, topo, dterms, laplacian=True, edge=True, normal=True, target_length=None):
    """vertices [B,V,3] float32, dterms [B,3] float64 -> Truth(values [B,3], grad [B,V,3], e_values [B,3],
    e_grad [B,V]), all float64."""
    e, f, src, dst, deg = index(topo)
    v = vertices.detach().double().clone().requires_grad_(True)
    B, V = v.shape[0], v.shape[1]
    g = dterms.double()
    values, parts = _evaluate(v, topo, laplacian, edge, normal, target_length)
    if values.requires_grad:
        (grad,) = torch.autograd.grad((values * g).sum(), v)
    else:
        grad = torch.zeros_like(v)
    values = values.detach()
    with torch.no_grad():
        e_values = torch.zeros(B, 3, dtype=torch.float64)
        a_lap, a_edge, a_nc = (torch.zeros(B, V, dtype=torch.float64) for _ in range(3))
        if "delta_len" in parts:
            dist = _norm(v[:, dst] - v[:, src])
            ring = _gather(B, V, src, dist) / deg.clamp(min=1)
            e_values[:, 0] = K_LAP * U * ring.sum(1) / V
            length = parts["delta_len"]
            w = torch.where(length > 0, 1.0 + ring / torch.where(length > 0, length, torch.ones_like(length)),
                            torch.zeros_like(length))
            a_lap = g[:, 0:1].abs() / V * (w + _gather(B, V, src, (w / deg.clamp(min=1))[:, dst]))
        if "edge_len" in parts:
            length = parts["edge_len"]
            E = e.shape[0]
            if target_length is None:
                per_value, per_grad = length, (length > 0).double()
            else:
                off = (length - float(target_length)).abs()
                per_value = 2.0 * length * off + off * off
                per_grad = torch.where(length > 0, 2.0 * (off + length), torch.zeros_like(length))
            e_values[:, 1] = K_EDGE * U * per_value.sum(1) / E
            a_edge = g[:, 1:2].abs() / E * _gather(B, V, src, torch.cat([per_grad, per_grad], 1))
        if "ok" in parts:
            F = f.shape[0]
            ok = parts["ok"]
            lp, lq, lr = _norm(parts["p"]), _norm(parts["q"]), _norm(parts["r"])
            l0, l1 = parts["l0"], parts["l1"]
            kappa = lp * lq / l0 + lr * lp / l1
            delta = U * kappa
            gap = _norm(parts["h0"] - parts["h1"])
            per = K_NC * (delta * gap + delta * delta) + 4.0 * U * parts["per"]
            e_values[:, 2] = torch.where(ok, per, torch.zeros_like(per)).sum(1) / F
            sin = _norm(torch.cross(parts["h0"], parts["h1"], dim=-1))
            levers = (_norm(parts["cb"]) / l0 + _norm(parts["db"]) / l1, lq / l0 + lr / l1, lp / l0, lp / l1)
            for role, lever in enumerate(levers):
                entry = torch.where(ok, (sin + kappa) * lever, torch.zeros_like(lever))
                a_nc = a_nc + g[:, 2:3].abs() / F * _gather(B, V, f[:, role], entry)
        e_grad = U * (K_GRAD_LAP * a_lap + K_GRAD_EDGE * a_edge + K_GRAD_NC * a_nc)
    return Truth(values, grad, e_values, e_grad)


def restatement32(vertices, topo, dterms, laplacian=True, edge=True, normal=True, target_length=None,
                  lap_form="difference", nc_form="half"):
    """The same formulas in float32 torch on the CPU, gradients by autograd -> (values [B,3], grad [B,V,3]) float32.
    lap_form "sum" and nc_form "cos" give the cancelling formulations the bounds exist to refuse."""
    v = vertices.detach().float().clone().requires_grad_(True)
    values, _ = _evaluate(v, topo, laplacian, edge, normal, target_length, lap_form, nc_form)
    if values.requires_grad:
        (grad,) = torch.autograd.grad((values * dterms.float()).sum(), v)
    else:
        grad = torch.zeros_like(v)
    return values.detach(), grad


def ratios(got_values, got_grad, want):
    """-> (err / E of the values [B,3], of the gradient [B,V]); 0 where both are 0, inf where only E is."""
    def ratio(err, bound):
        positive = bound > 0
        out = torch.where(positive, err / torch.where(positive, bound, torch.ones_like(bound)), err * float("inf"))
        return torch.where(err == 0, torch.zeros_like(out), out)
    verr = (got_values.detach().double().cpu() - want.values).abs()
    gerr = (got_grad.detach().double().cpu() - want.grad).norm(dim=-1)
    return ratio(verr, want.e_values), ratio(gerr, want.e_grad)


def caps(want, gradient_cap=EASY_GRADIENT):
    """-> (the share of vertices with E_v <= gradient_cap max|expected gradient|, the worst E_value / |value|)."""
    scale = float(want.grad.abs().max())
    share = float((want.e_grad <= gradient_cap * scale).double().mean())
    nonzero = want.values.abs() > 0
    loose = torch.where(nonzero, want.e_values / torch.where(nonzero, want.values.abs(), torch.ones_like(want.values)),
                        torch.zeros_like(want.values))
    return share, float(loose.max())


def check(got_values, got_grad, want, what, value_cap=1e-5, gradient_cap=EASY_GRADIENT, limit=1.0):
    """Every value within its E, every vertex's gradient within its own E_v, and the cap; the worst ratios are
    printed first.  -> (worst value err/E, worst gradient err/E)"""
    assert got_values.shape == want.values.shape and got_grad.shape == want.grad.shape, what
    assert bool(torch.isfinite(got_values).all()) and bool(torch.isfinite(got_grad).all()), "%s: not finite" % what
    rv, rg = ratios(got_values, got_grad, want)
    share, loose = caps(want, gradient_cap)
    worst_v, worst_g = float(rv.max()), float(rg.max())
    print("%s: values err/E %s, gradient worst err/E %.3f; share of vertices with E_v <= %g max|grad|: %.3f, "
          "worst E_value/|value| %.3g" % (what, ["%.3f" % float(x) for x in rv.max(0).values], worst_g, gradient_cap,
                                           share, loose))
    assert share >= EASY_SHARE, "%s: the gradient bound is loose on %.3f of the vertices" % (what, 1 - share)
    assert loose <= value_cap, "%s: a value bound is %.3g of its value, cap %.3g" % (what, loose, value_cap)
    assert worst_v <= limit, "%s: value err/E = %.3f" % (what, worst_v)
    assert worst_g <= limit, "%s: gradient err/E = %.3f at vertex %s" % (what, worst_g, int(rg.argmax()) % rg.shape[1])
    return worst_v, worst_g


# ---- the cases ------------------------------------------------------------------------------------------------------
def rotation():
    """One fixed generic rotation: the Q of a seeded 3 x 3 normal matrix."""
    g = torch.Generator().manual_seed(24)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    return q


def grid_triangles(rows, cols):
    out = []
    for i in range(rows - 1):
        for j in range(cols - 1):
            tl = i * cols + j
            out += [[tl, tl + cols, tl + 1], [tl + 1, tl + cols, tl + cols + 1]]
    return torch.tensor(out, dtype=torch.int32).reshape(-1, 3)


def grid(rows, cols, spacing, noise, seed, in_plane=0.0, scale_x=1.0, rotate=True, offset=(0.0, 0.0, 0.0)):
    """rows x cols vertices `spacing` apart in the plane z = 0, seeded normal noise of sigma `noise` out of the plane
    and `in_plane` within it, x scaled by scale_x, then the fixed rotation and the offset; float64 until the end."""
    g = torch.Generator().manual_seed(seed)
    i, j = torch.meshgrid(torch.arange(rows, dtype=torch.float64), torch.arange(cols, dtype=torch.float64), indexing="ij")
    v = torch.stack([j * spacing, i * spacing, torch.zeros_like(i)], -1).reshape(-1, 3)
    jitter = torch.randn(v.shape, generator=g, dtype=torch.float64)
    v = v + jitter * torch.tensor([in_plane, in_plane, noise], dtype=torch.float64)
    v = v * torch.tensor([scale_x, 1.0, 1.0], dtype=torch.float64)
    if rotate:
        v = v @ rotation().T
    v = v + torch.tensor(offset, dtype=torch.float64)
    return v.float()[None].contiguous(), grid_triangles(rows, cols)


def strip(V, seed=7):
    """A jittered triangle strip of V vertices (V - 2 triangles; none below three vertices)."""
    g = torch.Generator().manual_seed(seed + V)
    k = torch.arange(V, dtype=torch.float64)
    v = torch.stack([0.05 * torch.div(k, 2, rounding_mode="floor"), 0.05 * (k % 2), torch.zeros_like(k)], -1)
    v = (v + 0.01 * torch.randn(V, 3, generator=g, dtype=torch.float64)) @ rotation().T
    tri = [[i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2] for i in range(V - 2)]
    return v.float()[None].contiguous(), torch.tensor(tri, dtype=torch.int32).reshape(-1, 3)


def _runs(subsets, targets):
    out = []
    for (lap, edge, normal), target in itertools.product(subsets, targets):
        if target is not None and not edge:
            continue                                # the target only enters the edge term
        out.append(dict(laplacian=lap, edge=edge, normal=normal, target_length=target))
    return out


ALL, LAP, EDGE, NC = (True, True, True), (True, False, False), (False, True, False), (False, False, True)
EDGE_NC = (False, True, True)
EVERY_SUBSET = [s for s in itertools.product((False, True), repeat=3) if any(s)]
SPHERES = ["%s@%s" % (mesh, at) for mesh in ("sphere20", "sphere50") for at in OFFSETS]
FLAT = ["grid_1e-1@0", "grid_1e-1@100", "grid_1e-2@0", "grid_1e-2@100", "grid_1e-3@0", "grid_1e-3@100", "grid_1e-4@0"]
FLATTEST = "grid_1e-4@0"
STRIP_SIZES = [1, 2, 3, 7, 8, 9, 31, 32, 33, 64, 65]
FLAP_COUNTS = [255, 256, 257]
FAN_COUNTS = [6, 7, 8, 15, 16]                      # valence count + 1: 7, 8, 9, 16, 17
LAUNCH = (["strip_%d" % n for n in STRIP_SIZES] + ["flaps_%d" % n for n in FLAP_COUNTS] + ["grid_91"]
          + ["fan_%d" % (n + 1) for n in FAN_COUNTS])
CASES = SPHERES + FLAT + ["grid_planar", "sliver"] + LAUNCH + ["subsets"]

_cases = {}
_truths = {}


def sphere_vertices(name):
    """"sphere20": perturbed_sphere(20, 2, 0.05); "sphere50": shapes.sphere(1, 50) with sigma = 0.001 -> [B,V,3] f64"""
    if name == "sphere20":
        v, tri = ref.perturbed_sphere(20, 2, sigma=0.05, seed=3)
    else:
        v, tri = ref.perturbed_sphere(50, 1, sigma=0.001, seed=5)
    return v.double(), tri


def _cut_to_flaps(count):
    """The first triangles of a 24 x 24 jittered grid that give exactly `count` flaps (a triangle in the body of the
    grid closes two flaps at once, so where the count is stepped over one earlier triangle is left out as well)."""
    v, tri = grid(24, 24, 1.0 / 24, 0.01, seed=31, in_plane=0.008)
    for T in range(count // 2, tri.shape[0] + 1):
        have = len(ref.topology(tri[:T], v.shape[1])["flaps"])
        if have == count:
            return v, tri[:T].contiguous()
        if have > count:
            for drop in range(T - 2, -1, -1):
                cut = torch.cat([tri[:drop], tri[drop + 1:T]])
                if len(ref.topology(cut, v.shape[1])["flaps"]) == count:
                    return v, cut.contiguous()
    raise AssertionError("no cut of the grid has %d flaps" % count)


def _build(name):
    if name == "subsets":
        base, tri = sphere_vertices("sphere20")
        vertices = (base + torch.tensor(OFFSET, dtype=torch.float64)).float()
        runs = _runs(EVERY_SUBSET, (None, 0.05))
    elif name in SPHERES:
        mesh, at = name.split("@")
        base, tri = sphere_vertices(mesh)
        vertices = (base + torch.tensor(OFFSETS[at], dtype=torch.float64)).float()
        runs = _runs((ALL, LAP, EDGE, NC), (None, 0.05))
    elif name in FLAT:
        sigma, at = name[5:].split("@")
        vertices, tri = grid(24, 24, 1.0 / 24, float(sigma) / 24, seed=24, offset=OFFSETS[at])
        runs = _runs((ALL, EDGE_NC, NC), (None,))
    elif name == "grid_planar":
        vertices, tri = grid(24, 24, 1.0 / 24, 0.0, seed=24, rotate=False)
        runs = _runs((EDGE_NC,), (None,))
    elif name == "sliver":
        vertices, tri = grid(24, 24, 1.0 / 24, SLIVER_NOISE, seed=24, scale_x=SLIVER_SCALE)
        runs = _runs((EDGE_NC, NC), (None,))
    elif name.startswith("strip_"):
        vertices, tri = strip(int(name[6:]))
        runs = _runs((ALL,), (None, 0.05))
    elif name.startswith("flaps_"):
        vertices, tri = _cut_to_flaps(int(name[6:]))
        runs = _runs((ALL, NC), (None,))
    elif name == "grid_91":
        vertices, tri = grid(91, 91, 1.0 / 90, 0.3 / 90, seed=91, in_plane=0.3 / 90)
        runs = _runs((ALL, NC), (None,))
    elif name.startswith("fan_"):
        v, tri = ref.fan(int(name[4:]) - 1)
        vertices = torch.stack([v, v * torch.tensor([1.0, 0.8, 1.5])])
        runs = _runs((ALL,), (None, 0.05))
    else:
        raise KeyError(name)
    B = vertices.shape[0]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    dterms = torch.randn(B, 3, generator=g, dtype=torch.float64)
    if name == "subsets":                           # an upstream gradient with a zero and a negative entry
        dterms[0, 0], dterms[0, 1] = 0.0, -abs(dterms[0, 1])
        dterms[1, 2], dterms[1, 0] = 0.0, -abs(dterms[1, 0])
    return Case(vertices.contiguous(), tri, ref.topology(tri, vertices.shape[1]), dterms, runs)


# The sliver: the grid squeezed 1:256 along one in-plane axis, noise 1.5 squeezed cells out of the plane (the triangles
# stay thin: kappa reaches 256 in a quarter of the flaps' corners, theta is about 1).  The most extreme power of two
# that keeps the default caps: E_nc / nc = 2 K_NC u (kappa0 + kappa1) / theta <= 1e-5 needs kappa0 + kappa1 <= 170
# theta, so kappa = 1e3 would need theta = 12 rad; at 1:512 the value bound is 1.3e-5 of the value.
SLIVER_SCALE = 1.0 / 256
SLIVER_NOISE = 1.5 * SLIVER_SCALE / 24
# (value cap, gradient cap) per (case, run) where the defaults 1e-5 and 1e-4 cannot hold: the first decade that does.
# Everything not listed keeps the defaults -- the sliver and the grids at sigma = 1e-1 among them.
#   value: E_nc / nc >= 2 K_NC u (kappa0 + kappa1) / theta, 5.0e-5 at sigma = 1e-3 and 4.9e-4 at 1e-4 (that one is
#          the exception the cases were given from the start);
#   gradient, the normal term: K_GRAD_NC u (kappa0 + kappa1) / theta of the normal term's own scale (the run "n");
#          next to the edge term ("en") it is measured against the edge gradient's scale, whatever theta is;
#   gradient, the Laplacian ("len"): w_i = 1 + r_i / |delta_i| is 1e1 .. 1e4 on these regular grids.  Its VALUE bound
#          does not depend on w_i and stays at the default cap.
CAPS = {
    ("grid_1e-2@0", "len"): (1e-5, 1e-3), ("grid_1e-2@100", "len"): (1e-5, 1e-3),
    ("grid_1e-3@0", "len"): (1e-4, 1e-2), ("grid_1e-3@100", "len"): (1e-4, 1e-2),
    ("grid_1e-3@0", "en"): (1e-4, 1e-3), ("grid_1e-3@100", "en"): (1e-4, 1e-3),
    ("grid_1e-3@0", "n"): (1e-4, 1e-3), ("grid_1e-3@100", "n"): (1e-4, 1e-3),
    ("grid_1e-4@0", "len"): (1e-3, 1e-1), ("grid_1e-4@0", "en"): (1e-3, 1e-3), ("grid_1e-4@0", "n"): (1e-3, 1e-2),
    ("grid_planar", "en"): (1e-5, 1e-3),
}


def caps_of(name, run):
    """-> (value cap, gradient cap) of one run of a case"""
    return CAPS.get((name, run_key(run)), (1e-5, EASY_GRADIENT))


def case(name):
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


def run_key(run):
    return "".join(c for c, on in zip("len", (run["laplacian"], run["edge"], run["normal"])) if on) + (
        "" if run["target_length"] is None else "@%g" % run["target_length"])


def truth_of(name, run):
    """truth(case(name), **run), computed once and shared."""
    key = (name, run_key(run))
    if key not in _truths:
        c = case(name)
        _truths[key] = truth(c.vertices, c.topo, c.dterms, **run)
    return _truths[key]


def forward_rows(V, F, laplacian, edge, normal):
    """The workspace rows one image's forward launch writes: its vertex blocks and its flap blocks."""
    vertex_blocks = -(-V // VERTICES_PER_BLOCK) if (laplacian or edge) else 0
    flap_blocks = -(-F // FLAPS_PER_BLOCK) if normal else 0
    return vertex_blocks + flap_blocks
