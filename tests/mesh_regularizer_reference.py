"""Float64 restatement of the mesh regularisers ("Mesh regularisers"), written from the
definitions: the topology by plain Python loops over sets and dictionaries, the terms by torch float64 with
autograd.  Shares nothing with the package's topology code or kernels."""
import torch

NORMAL_FLOOR = 1e-8


def topology(triangles, vertex_count):
    """-> dict: edges [(lo, hi)] ascending, neighbours {vertex: sorted list}, flaps [(a, b, c, d)] in the edges'
    order, boundary / nonmanifold: the edges with one / more than two (triangle, side) rows."""
    V = int(vertex_count)
    rows = {}                                   # (lo, hi) -> opposite corners, in (triangle, side) order
    for tri in [[int(i) for i in t] for t in triangles.tolist()]:
        if any(i < 0 or i >= V for i in tri):
            continue                            # dropped whole
        for k in range(3):
            p, q = tri[(k + 1) % 3], tri[(k + 2) % 3]
            if p == q:
                continue                        # no edge
            rows.setdefault((min(p, q), max(p, q)), []).append(tri[k])
    edges = sorted(rows)
    neighbours = {v: set() for v in range(V)}
    for lo, hi in edges:
        neighbours[lo].add(hi)
        neighbours[hi].add(lo)
    flaps = []
    for lo, hi in edges:
        opposite = rows[(lo, hi)]
        if len(opposite) != 2:
            continue
        c, d = opposite
        if c in (lo, hi) or d in (lo, hi):
            continue
        flaps.append((lo, hi, c, d))
    return {"V": V, "edges": edges, "neighbours": {v: sorted(n) for v, n in neighbours.items()}, "flaps": flaps,
            "boundary": [e for e in edges if len(rows[e]) == 1],
            "nonmanifold": [e for e in edges if len(rows[e]) > 2]}


def _norm(x):
    """|x| over the last axis, gradient 0 at x = 0."""
    sq = (x * x).sum(-1)
    nonzero = sq > 0
    return torch.where(nonzero, torch.sqrt(torch.where(nonzero, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def terms(vertices, topo, laplacian=True, edge=True, normal=True, target_length=None):
    """vertices [B,V,3] (any dtype, evaluated in float64) -> [B,3] float64 (lap, edge, nc); a term switched off is 0."""
    v = vertices.double()
    B, V = v.shape[0], v.shape[1]
    assert V == topo["V"]
    zero = v.new_zeros(B)
    lap, edg, nc = zero, zero, zero
    if laplacian:
        total = v.new_zeros(B)
        for i in range(V):
            ring = topo["neighbours"][i]
            if not ring:
                continue                        # a vertex without neighbours contributes 0
            delta = v[:, ring].sum(1) / len(ring) - v[:, i]
            total = total + _norm(delta)
        lap = total / V
    if edge and topo["edges"]:
        e = torch.tensor(topo["edges"], dtype=torch.long)
        length = _norm(v[:, e[:, 0]] - v[:, e[:, 1]])
        edg = (length if target_length is None else (length - float(target_length)) ** 2).sum(1) / len(topo["edges"])
    if normal and topo["flaps"]:
        f = torch.tensor(topo["flaps"], dtype=torch.long)
        a, b, c, d = v[:, f[:, 0]], v[:, f[:, 1]], v[:, f[:, 2]], v[:, f[:, 3]]
        n0 = torch.cross(b - a, c - a, dim=-1)
        n1 = torch.cross(d - a, b - a, dim=-1)
        l0, l1 = _norm(n0), _norm(n1)
        ok = (l0 > NORMAL_FLOOR) & (l1 > NORMAL_FLOOR)
        cos = (n0 * n1).sum(-1) / torch.where(ok, l0 * l1, torch.ones_like(l0))
        nc = torch.where(ok, 1.0 - cos, torch.zeros_like(cos)).sum(1) / len(topo["flaps"])
    return torch.stack([lap, edg, nc], dim=1)


def gradients(vertices, topo, dterms, **kwargs):
    """-> (terms [B,3], d(sum(terms * dterms)) / d vertices [B,V,3]), float64."""
    v = vertices.detach().double().clone().requires_grad_(True)
    out = terms(v, topo, **kwargs)
    if not out.requires_grad:                   # no term asked for (or nothing to sum): the gradient is 0
        return out, torch.zeros_like(v)
    (grad,) = torch.autograd.grad((out * dterms.double()).sum(), v)
    return out.detach(), grad


def odd_mesh():
    """One mesh with every irregular case (vertices [10,3] float32, triangles [T,3] int32):
      vertices 0..3   a bent manifold flap across the edge (0, 1): triangles (0,1,2) and (1,0,3)
      edge (1, 2)     shared by three triangles: (0,1,2), (1,2,4), (2,1,5) -- non-manifold, no flap
      boundary edges  e.g. (0, 3), (1, 3), (2, 4)
      vertex 9        isolated
      (4, 4, 5)       a triangle that repeats an index: its edge (4, 5) has two rows with opposite corner 4
      (0, 1, 12)      an index >= V: dropped whole
      (2, 6, 7) twice a duplicated triangle: flaps with c == d
      vertices 6, 8   edge-connected and at the same position (a zero-length edge, through triangle (6, 8, 7))
      (3, 5, 8)...    vertices 3, 5 and 8 = 6 are collinear: triangle (3, 5, 8) has zero area, and it lies in a flap
                      across the edge (3, 5) with triangle (5, 3, 0)"""
    vertices = torch.tensor([
        [0.0, 0.0, 0.0],      # 0
        [1.0, 0.0, 0.0],      # 1
        [0.5, 1.0, 0.2],      # 2
        [0.5, -1.0, 0.5],     # 3
        [1.5, 1.0, -0.3],     # 4
        [1.5, 0.0, 0.5],      # 5   (3 + 5) / 2 ... see vertex 8
        [2.5, 1.0, 0.5],      # 6   = 3 + 2 * (5 - 3): collinear with 3 and 5
        [2.0, 2.0, 0.0],      # 7
        [2.5, 1.0, 0.5],      # 8   the same position as 6
        [5.0, 5.0, 5.0],      # 9   isolated
    ], dtype=torch.float32)
    triangles = torch.tensor([
        [0, 1, 2], [1, 0, 3], [1, 2, 4], [2, 1, 5], [4, 4, 5], [0, 1, 12], [2, 6, 7], [2, 6, 7], [6, 8, 7],
        [3, 5, 8], [5, 3, 0],
    ], dtype=torch.int32)
    return vertices, triangles


def fan(count=70):
    """`count` triangles around vertex 0 (an open fan on a cone, V = count + 2): valence count + 1."""
    angle = torch.arange(count + 1, dtype=torch.float64) * (5.5 / count)
    radius = 1.0 + 0.1 * torch.sin(7.0 * angle)
    rim = torch.stack([radius * torch.cos(angle), radius * torch.sin(angle), 0.3 + 0.05 * torch.cos(3.0 * angle)], 1)
    vertices = torch.cat([torch.zeros(1, 3, dtype=torch.float64), rim]).float()
    triangles = torch.tensor([[0, i + 1, i + 2] for i in range(count)], dtype=torch.int32)
    return vertices, triangles


def perturbed_sphere(resolution, batch, sigma=0.05, seed=0):
    """shapes.sphere(1, resolution) with a different seeded perturbation per image -> ([B,V,3] f32, triangles)."""
    from pytorch_mesh_renderer_amd.common import shapes
    vertices, triangles, _ = shapes.sphere(1.0, resolution)
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(batch, vertices.shape[0], 3, generator=g) * sigma
    return (vertices[None] + noise).float().contiguous(), triangles
