"""A float64 truth for the SoftRas kernels (csrc/soft.hip), the scenes it is evaluated on and the rule
that says which pixels it cannot judge (TEST INFRASTRUCTURE ONLY).

Truth: oracle/soft.py follows the dtype of its inputs; fed the float32 leaves cast to float64 it evaluates
the same piecewise function at the float32 pixel centres the kernels use, with torch autograd for the
gradients.  The yardstick of every bound is the float32 run of the same restatement against that truth,
on the same scene, mask and upstream weights:

    ref_err = max|f32 - f64| / max|f64|        (per tensor; the image counts as one)

and a kernel is allowed  K * ref_err + FLOOR  per tensor, relative to max|f64| (allowed()).

Borderline rule: SoftRas is piecewise -- inside / outside, which edge is nearest, the blur cull, the depth
cull, the bbox test, the clamps of t and n.l -- and two float evaluations may decide differently, or sit on
a gradient kink, within rounding of a boundary.  borderline() marks a pixel when a relevant pair of it is
within tol of one.  Marked pixels are left out of the image comparison and get ZERO upstream gradient in
every backward (truth, restatement, kernel), so the gradient comparison needs no exclusion of its own.
Two refinements of the rule as first stated.  (1) The near-tie of the two smallest edge distances and the
clamp of t are tested for inside pairs too: an inside pair's coverage D = sigmoid(+d^2 / sigma) differentiates
through its nearest edge like an outside pair's.  (2) A tie between two edges that are both clamped onto the
vertex they share is no decision (_same_vertex_tie): that is every pair of a corner fan, rounding alone names
the edge, and value and gradient are the same either way; evaluations are compared by feature() there.

Scenes: scene(name) builds each from a seed; SCENES lists them.  All leaves are random (clip is the
projected mesh, w varying per vertex; world / normals are the mesh's jittered, so that no leaf is a
function of another).
"""
import functools

import torch

from oracle import soft as oracle_soft
from pytorch_mesh_renderer_amd.common import synthetic

TOL = 1e-5      # borderline distance: ~100 float32 ulps of an NDC coordinate, a barycentric or a depth
FLOOR = 1e-7    # covers tensors whose ref_err happens to be a few ulps
K = 8           # worst measured got_err / ref_err over all runs, scenes and tensors (4.8), rounded up to a power of two
CAP = 0.05      # at most this share of a scene's pixels may be borderline
OLD_ATOL = 1e-4
LEAVES = ("clip", "world", "normals", "diffuse", "lpos", "lint")
kTile, kListCap, kCell = 16, 512, 128   # csrc/soft.hip: kTile, kListCap, kCellTiles * kTile


def _same_vertex_tie(trace, tol):
    """bool [P,T]: the two nearest edges are both clamped, by more than tol, onto the vertex they share.  In a
    corner fan that is every pair -- both distances ARE the distance to that vertex, and which edge the argmin
    names is decided by rounding -- and it is harmless: either edge gives the same barycentrics (the vertex's),
    the same squared distance and, the clamp passing nothing, the same gradient (all of it to that vertex)."""
    e = torch.arange(3)
    tr = trace["t_raw_edges"]
    vertex = torch.where(tr > 1 + tol, (e + 1) % 3, torch.where(tr < -tol, e, torch.full_like(e, -1)))   # [P,T,3]
    order = trace["edge_dist"].argsort(-1)
    va, vb = vertex.gather(-1, order[..., :1])[..., 0], vertex.gather(-1, order[..., 1:2])[..., 0]
    return (va >= 0) & (va == vb)


def feature(trace):
    """int [P,T]: what the nearest point lies on -- edge 0..2, or 3 + v for vertex v (the edge named by the argmin
    is clamped onto it).  Two evaluations that name different edges of a corner fan agree on this."""
    e, t = trace["edge"], trace["t_raw"]
    return torch.where(t > 1, 3 + (e + 1) % 3, torch.where(t < 0, 3 + e, e))


def borderline(trace, blur, tol=TOL):
    """trace of a float64 oracle call -> bool [P]: pixels with a relevant pair within tol of a decision."""
    bc, sq, dist, z, p2 = trace["bc"], trace["sq_dist"], trace["edge_dist"], trace["z"], trace["p2"]
    lo, hi = trace["lo"], trace["hi"]
    front = (trace["valid"] & (trace["area"] < 0))[None, :]
    maybe_in = (bc > -tol).all(-1)
    relevant = front & (maybe_in | (sq <= blur ** 2 * (1 + tol)))
    near_bbox = (((p2[:, None, 0] - lo[None, :, 0]).abs() < tol) | ((p2[:, None, 0] - hi[None, :, 0]).abs() < tol) |
                 ((p2[:, None, 1] - lo[None, :, 1]).abs() < tol) | ((p2[:, None, 1] - hi[None, :, 1]).abs() < tol))
    near_in = maybe_in & (bc.abs() < tol).any(-1)
    near_blur = ~maybe_in & ((sq - blur ** 2).abs() < tol * blur ** 2)
    s = dist.sort(-1).values
    near_tie = ((s[..., 1] - s[..., 0]) < tol * s[..., 1].clamp(min=1e-30)) & ~_same_vertex_tie(trace, tol)
    near_z = (z.abs() < tol) | ((z - 1).abs() < tol)
    t = trace["t_raw"]
    near_t = (t.abs() < tol) | ((t - 1).abs() < tol)
    ndl = trace["ndl_raw"]
    near_ndl = ((ndl.abs() < tol) | ((ndl - 1).abs() < tol)).any(-1)
    return (relevant & (near_bbox | near_in | near_blur | near_tie | near_z | near_t | near_ndl)).any(-1)


def _oracle(leaves, tri, W, H, params, trace=None):
    return oracle_soft.rasterize_batch(leaves["clip"], tri, leaves["world"], leaves["normals"], leaves["diffuse"],
                                       leaves["lpos"], leaves["lint"], W, H, *params, trace=trace)


def rel_err(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


def allowed(ref_err, k=None):
    return (K if k is None else k) * ref_err + FLOOR


class Truth:
    """One image: the float64 truth, its borderline mask, the masked upstream weights, and the float32
    restatement's error against it.  leaves: float32 CPU tensors by LEAVES name."""

    def __init__(self, leaves, tri, W, H, params, seed=0, signed=True):
        self.leaves = {k: leaves[k].detach().clone().float() for k in LEAVES}
        self.tri, self.W, self.H, self.params = tri, W, H, tuple(params)
        self.trace, self.trace32 = {}, {}
        image, grads = self._run(torch.float64, None, self.trace)
        self.image = image
        self.bad = borderline(self.trace, params[2]).reshape(H, W)
        self.image32, _ = self._run(torch.float32, None, self.trace32)
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn if signed else torch.rand)(H, W, 4, generator=g, dtype=torch.float64) / (H * W * 4)
        self.weights = self.masked(w)
        self.grads, self.ref_err = self.evaluate(self.weights)

    def masked(self, w):
        w = w.clone()
        w[self.bad] = 0
        return w

    def _run(self, dtype, weights, trace=None):
        lv = {k: v.to(dtype).clone().requires_grad_(True) for k, v in self.leaves.items()}
        img = _oracle(lv, self.tri, self.W, self.H, self.params, trace)
        if weights is None:
            return img.detach(), None
        grads = torch.autograd.grad((img * weights.to(dtype)).sum(), [lv[k] for k in LEAVES], allow_unused=True)
        return img.detach(), {k: (torch.zeros_like(lv[k]) if g is None else g).detach() for k, g in zip(LEAVES, grads)}

    def evaluate(self, weights):
        """weights [H,W,4] float64, zero on borderline pixels -> (truth gradients, ref_err by tensor + image)."""
        assert not bool((weights[self.bad] != 0).any())
        _, g64 = self._run(torch.float64, weights)
        _, g32 = self._run(torch.float32, weights)
        ref = {k: rel_err(g32[k], g64[k]) for k in LEAVES}
        ref["image"] = self.image_err(self.image32)
        return g64, ref

    def image_err(self, got):
        ok = ~self.bad
        return float((got.double()[ok] - self.image[ok]).abs().max() / self.image[ok].abs().max())

    def decisions_differ(self):
        """bool [H,W]: pixels where the float32 restatement decided otherwise than the truth."""
        a, b = self.trace, self.trace32
        same = (a["keep"] == b["keep"]) & (~a["keep"] | ((a["inside"] == b["inside"]) & (feature(a) == feature(b))))
        return ~same.all(-1).reshape(self.H, self.W)


def compare(label, truth, got_image, got_grads, want_grads=None, ref_err=None, k=None):
    """Prints got_err / ref_err per tensor and returns the list of tensors over the bound (empty = pass)."""
    want_grads = truth.grads if want_grads is None else want_grads
    ref_err = truth.ref_err if ref_err is None else ref_err
    got = {name: rel_err(got_grads[name], want_grads[name]) for name in LEAVES}
    if got_image is not None:
        got["image"] = truth.image_err(got_image)
    over = []
    for name, e in got.items():
        bound = allowed(ref_err[name], k)
        print("%-28s %-8s got_err %.3g  ref_err %.3g  ratio %.3g  allowed %.3g  max|truth| %.3g" % (
            label, name, e, ref_err[name], e / max(ref_err[name], 1e-300), bound,
            1.0 if name == "image" else float(want_grads[name].abs().max())))
        if not e <= bound:
            over.append("%s %s: %.3g > %.3g" % (label, name, e, bound))
    return over


def absolute_bounds(truth, want_grads=None, ref_err=None, k=None):
    """The absolute error the bound allows per gradient tensor (the condition: below today's 1e-4)."""
    want_grads = truth.grads if want_grads is None else want_grads
    ref_err = truth.ref_err if ref_err is None else ref_err
    return {name: allowed(ref_err[name], k) * float(want_grads[name].abs().max()) for name in LEAVES}


# ---- scenes ---------------------------------------------------------------------------------------------------------

_LIGHTS = [[0.5, 1.0, 3.0], [-2.0, 0.3, 2.0], [3.0, 0.2, 0.3]]   # the third grazes: n.l < 0 on the far half


def _sphere_leaves(seed, W, H, n, L, aligned_light=False):
    job = synthetic.sphere_job(1, W, H, n)
    g = torch.Generator().manual_seed(seed)
    V = job["vertices"].shape[1]
    world = job["vertices"][0] + 0.05 * torch.randn(V, 3, generator=g)
    normals = job["normals"][0] + 0.2 * torch.randn(V, 3, generator=g)
    lpos = torch.tensor(_LIGHTS)[:L] + 0.1 * torch.randn(min(L, 3), 3, generator=g)
    if aligned_light:
        # a light on the normal ray of the vertex that faces the camera (eye (0, 0, 3)): n.l -> 1 there
        v = int(job["vertices"][0][:, 2].argmax())
        lpos = torch.cat([lpos, (world[v] + 2.0 * torch.nn.functional.normalize(normals[v], dim=0))[None]])
    L = lpos.shape[0]
    return {"clip": job["clip"][0].clone(), "world": world, "normals": normals,
            "diffuse": 0.1 + 0.8 * torch.rand(V, 3, generator=g), "lpos": lpos,
            "lint": 0.4 + 0.6 * torch.rand(L, generator=g)}, job["triangles"]


def _crafted():
    """A dozen hand-placed triangles at 40 x 24 (NDC x, y, z per vertex; counter-clockwise = front-facing)."""
    g = torch.Generator().manual_seed(41)
    xyz = torch.tensor([
        [-0.90, -0.80, 0.20], [-0.10, -0.70, 0.30], [-0.50, 0.60, 0.10],      # 0-2   layer A (nearest)
        [-0.80, -0.60, 0.50], [0.00, -0.50, 0.60], [-0.40, 0.70, 0.55],       # 3-5   layer B
        [-0.85, -0.30, -0.30], [-0.05, -0.75, -0.20], [-0.30, 0.50, -0.40],   # 6-8   layer C
        [0.20, -0.60, 0.10], [0.80, -0.50, 0.30], [0.70, 0.30, 0.20], [0.15, 0.20, 0.40],   # 9-12  quad: two triangles
        [0.10, 0.40, 0.60], [0.60, 0.50, 1.50], [0.30, 0.90, 0.80],           # 13-15 depth-culled towards vertex 14
        [0.70, -0.90, 0.00], [1.40, -0.80, 0.10], [0.90, -0.20, 0.05],        # 16-18 partly off the image
        [-0.10, 0.75, 0.00], [0.00, 0.78, 0.10], [-0.06, 0.88, 0.05],         # 19-21 small: mostly corner fans
        [-0.95, 0.55, -0.50], [-0.70, 0.95, -0.60], [-0.60, 0.60, -0.55],     # 22-24 wound clockwise: back-facing
        [0.25, 0.25, 0.10], [0.50, 0.50, 0.10], [0.75, 0.75, 0.10],           # 25-27 collinear: zero area, w = 1 exactly
    ])
    xyz[:25, :2] += 0.01 * (2 * torch.rand(25, 2, generator=g) - 1)           # off every pixel centre and round number
    tri = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [9, 11, 12], [13, 14, 15], [16, 17, 18],
                        [19, 20, 21], [22, 23, 24], [25, 26, 27]], dtype=torch.int32)
    V = xyz.shape[0]
    w = 0.8 + 0.8 * torch.rand(V, 1, generator=g)
    w[25:] = 1.0   # x = y and the row of ones stay exact: the matrix is singular in every precision
    leaves = {"clip": torch.cat([xyz * w, w], -1), "world": torch.randn(V, 3, generator=g) * 0.5,
              "normals": torch.randn(V, 3, generator=g), "diffuse": 0.1 + 0.8 * torch.rand(V, 3, generator=g),
              "lpos": torch.tensor([[0.5, 1.0, 3.0], [-2.0, 0.3, 2.0]]), "lint": torch.tensor([0.9, 0.6])}
    return leaves, tri


DEFAULT, SOFT = (1e-5, 1e-4, 0.01), (3e-4, 5e-3, 0.03)
SCENES = ("sphere-default", "sphere-soft", "lights-3", "lights-4", "two-walks", "two-cells", "crafted",
          "batch-2a", "batch-2b")
SOFTER = tuple(n for n in SCENES if n != "sphere-default")   # the scenes the "below 1e-4 absolute" condition covers


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (leaves, triangles, W, H, (sigma, gamma, blur))."""
    if name == "sphere-default":
        return _sphere_leaves(1, 48, 40, 8, 1) + (48, 40, DEFAULT)
    if name == "sphere-soft" or name == "batch-2a":
        return _sphere_leaves(2, 48, 40, 8, 2) + (48, 40, SOFT)
    if name == "batch-2b":   # the same mesh: other vertices, attributes and lights
        leaves, tri = _sphere_leaves(7, 48, 40, 8, 2)
        g = torch.Generator().manual_seed(8)
        leaves["clip"] = leaves["clip"] * (1.0 + 0.1 * torch.rand(leaves["clip"].shape[0], 1, generator=g))
        leaves["clip"][:, :2] += 0.15
        leaves["lpos"] = torch.tensor([[-1.0, 2.0, 2.5], [1.5, -0.5, 3.0]])
        return leaves, tri, 48, 40, SOFT
    if name == "lights-3":
        return _sphere_leaves(3, 48, 40, 8, 3) + (48, 40, SOFT)
    if name == "lights-4":
        return _sphere_leaves(4, 48, 40, 8, 3, aligned_light=True) + (48, 40, SOFT)
    if name == "two-walks":
        return _sphere_leaves(5, 16, 16, 32, 1) + (16, 16, (1e-4, 1e-3, 0.02))
    if name == "two-cells":
        return _sphere_leaves(6, 144, 136, 6, 2) + (144, 136, (1e-4, 1e-3, 0.02))
    if name == "crafted":
        return _crafted() + (40, 24, (5e-3, 5e-2, 0.12))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def truth(name):
    leaves, tri, W, H, params = scene(name)
    return Truth(leaves, tri, W, H, params, seed=sum(map(ord, name)))


# ---- liveness: what the trace says about the kernel's regimes --------------------------------------------------------

def _centre_x(x, W):
    return torch.tensor(2.0 * ((x + 0.5) / W) - 1.0, dtype=torch.float32).double()


def _centre_y(y, H):
    return torch.tensor(-2.0 * ((y + 0.5) / H) + 1.0, dtype=torch.float32).double()


def tile_hits(t):
    """Valid bbox hits per 16 x 16 tile, with tile_geometry's rectangle expressions (csrc/soft.hip) -> list."""
    tr = t.trace
    front = tr["valid"] & (tr["area"] < 0)
    out = []
    for ty in range((t.H + kTile - 1) // kTile):
        for tx in range((t.W + kTile - 1) // kTile):
            x0, y0 = tx * kTile, ty * kTile
            x1, y1 = min(x0 + kTile, t.W) - 1, min(y0 + kTile, t.H) - 1
            tx0, tx1 = _centre_x(x0, t.W), _centre_x(x1, t.W)
            ty1, ty0 = _centre_y(y0, t.H), _centre_y(y1, t.H)      # y grows downwards in the image
            hit = front & (tr["lo"][:, 0] <= tx1) & (tr["hi"][:, 0] >= tx0) & (tr["lo"][:, 1] <= ty1) & (tr["hi"][:, 1] >= ty0)
            out.append(int(hit.sum()))
    return out


def straddles(t):
    """-> (triangles whose inflated bbox straddles x-pixel 128 with clean kept pairs on both sides, same for y)."""
    tr = t.trace
    keep = (tr["keep"] & ~t.bad.reshape(-1, 1)).reshape(t.H, t.W, -1)
    bx = (tr["lo"][:, 0] < _centre_x(kCell - 1, t.W)) & (tr["hi"][:, 0] > _centre_x(kCell, t.W))
    by = (tr["hi"][:, 1] > _centre_y(kCell - 1, t.H)) & (tr["lo"][:, 1] < _centre_y(kCell, t.H))
    kx = keep[:, :kCell].any(0).any(0) & keep[:, kCell:].any(0).any(0)
    ky = keep[:kCell].any(0).any(0) & keep[kCell:].any(0).any(0)
    return int((bx & kx).sum()), int((by & ky).sum())


def crafted_classes(t):
    """Crafted scene -> ({class: clean kept pairs [P,T]}, {class: pixels [H,W] that carry the class's weights}).
    Pixel classes of the outside branches hold no inside pair, so that those branches are not buried."""
    tr = t.trace
    clean = ~t.bad.reshape(-1, 1)
    keep = tr["keep"] & clean
    ins, out = keep & tr["inside"], keep & ~tr["inside"]
    free = (tr["t_raw"] > 0) & (tr["t_raw"] < 1)
    pairs = {"inside": ins, "corner-t0": out & (tr["t_raw"] < 0), "corner-t1": out & (tr["t_raw"] > 1)}
    for e in range(3):
        pairs["edge-%d" % e] = out & free & (tr["edge"] == e)
    zr = torch.where(keep, tr["z"], torch.full_like(tr["z"], -1.0))
    distinct = torch.tensor([len(set(r[r >= 0].tolist())) for r in zr])
    layered = (keep.sum(-1) >= 3) & (distinct >= 3)
    pairs["layers"] = keep & layered[:, None]
    # culled by depth alone on a triangle that is kept elsewhere; a triangle that leaves the image
    would = tr["cand"] & clean & (tr["inside"] | (tr["sq_dist"] <= t.params[2] ** 2))
    pairs["depth-culled"] = would & ((tr["z"] < 0) | (tr["z"] > 1)) & keep.any(0)[None, :]
    off = (tr["hi"] - t.params[2] > 1).any(-1) | (tr["lo"] + t.params[2] < -1).any(-1)
    pairs["partly-off-image"] = keep & off[None, :]
    hw = lambda m: m.reshape(t.H, t.W)
    no_inside = ~ins.any(-1)
    pixels = {"inside": hw(ins.any(-1) & ~out.any(-1)), "layers": hw(layered),
              "corners": hw((pairs["corner-t0"] | pairs["corner-t1"]).any(-1) & no_inside)}
    for e in range(3):
        pixels["edge-%d" % e] = hw(pairs["edge-%d" % e].any(-1) & no_inside)
    return pairs, pixels


def class_weights(t, pixels):
    """The scene's upstream weights restricted to a pixel class."""
    w = t.weights.clone()
    w[~pixels] = 0
    return w


@functools.lru_cache(maxsize=None)
def crafted_class_truths():
    """-> {pixel class: (weights, truth gradients, ref_err)} of the crafted scene, one backward per class."""
    t = truth("crafted")
    out = {}
    for name, pixels in crafted_classes(t)[1].items():
        w = class_weights(t, pixels)
        out[name] = (w,) + t.evaluate(w)
    return out


# ---- the kernels ---------------------------------------------------------------------------------------------------

def kernel_run(truths, device, weights=None, mode="autograd"):
    """One launch over the images of `truths` (a list: the batch) -> [(image, gradients by LEAVES name)], float32
    CPU.  mode: 'autograd' (soft_mesh_renderer.rasterize), 'native' (_native.soft_forward / soft_backward, records
    rebuilt by the backward) or 'prepared' (the forward's kept records handed to the backward)."""
    from pytorch_mesh_renderer_amd import _native
    from pytorch_mesh_renderer_amd.soft_mesh_renderer import rasterize as soft_rasterize
    t0 = truths[0]
    weights = [t.weights for t in truths] if weights is None else weights
    drgba = torch.stack(weights).float().to(device)
    stacked = {k: torch.stack([t.leaves[k] for t in truths]).to(device) for k in LEAVES}
    tri = t0.tri.to(device)
    sigma, gamma, blur = t0.params
    if mode == "autograd":
        lv = {k: v.requires_grad_(True) for k, v in stacked.items()}
        if len(truths) == 1:
            img = soft_rasterize.rasterize_batch(lv["clip"][0], tri, lv["world"][0], lv["normals"][0], lv["diffuse"][0],
                                                 lv["lpos"][0], lv["lint"][0], t0.W, t0.H, sigma, gamma, blur)[None]
        else:
            img = soft_rasterize.SoftRasterizer.apply(lv["clip"], lv["world"], lv["normals"], lv["diffuse"], tri,
                                                      lv["lpos"], lv["lint"], t0.W, t0.H, sigma, gamma, blur)
        (img * drgba).sum().backward()
        grads = {k: lv[k].grad for k in LEAVES}
    else:
        args = (stacked["clip"], stacked["world"], stacked["normals"], stacked["diffuse"], tri, stacked["lpos"],
                stacked["lint"])
        out = _native.soft_forward(*args, t0.W, t0.H, sigma, gamma, blur, keep_prepared=(mode == "prepared"))
        img, aux = out[0], out[1]
        dclip, dpos, dnrm, ddif, dlp, dli = _native.soft_backward(
            drgba, img, aux, *args, sigma, gamma, blur, prepared=(out[2] if mode == "prepared" else None))
        grads = {"clip": dclip, "world": dpos, "normals": dnrm, "diffuse": ddif, "lpos": dlp, "lint": dli}
    return [(img[b].detach().cpu(), {k: grads[k][b].detach().cpu() for k in LEAVES}) for b in range(len(truths))]
