"""Seeded scenes for the antialiasing truth tests, each named for the regime of k_aa_forward / k_aa_backward
(csrc/antialias.hip: 64 x 4 pixel workgroups, one wavefront per row) it is built to reach.

A scene is inputs only: clip, triangles, the image size and, for a FOREIGN scene, an edit of the G-buffer, the
triangles or the topology that makes them stop belonging to one another.  The G-buffer comes from whoever asks:
oracle.forward on the host (host()), _native.rasterize_forward on the device (the GPU tests hand theirs to
assemble()).  tests/test_antialias_truth_host.py asserts that each scene reaches its regime.

  ragged_WxH    the cube from two cameras at sizes no tile fits: lanes and whole wavefronts out of range
  seams_*       a sphere and a soup at 130 x 10: many vertices per wavefront, pairs across ix 63|64 and iy 3|4
  long_edge     a square at 128 x 8 whose outline runs along rows and columns: whole wavefronts on two vertices
  spike         one triangle over one pixel centre: mask 15, a vertex in several slots of one lane, opposite -1
  midpoint      the square's outline on pixel boundaries: every candidate has t == 0.5, nothing blends
  centre        ... through pixel centres: every candidate blends with t == 0 and weight 0.5
  coplanar      two overlapping triangles at one depth: rule 3's equal-z, larger-id tie
  rolled_1 / 2  the cube's G-buffer moved by one / two pixels: t clamped to 0 and to 1
  poisoned      ... with ids T, T + 7, -1, INT32_MIN, a triangle naming vertex V, an opposite entry V + 3
  scaled_*      soup 1 with clip times 2^-6 and 2^5 (and scaled_1, the same soup unscaled)
  no_triangles  T = 0 under an all-zero G-buffer;  no_images: B = 0
"""
import functools

import numpy as np
import torch

import antialias_reference as ref
from pytorch_mesh_renderer_amd.common import camera_utils, shapes, synthetic

INT32_MIN = -2 ** 31
K = 16.0            # the bound's rounding count: 4 r32 rounded up to a power of two (test_antialias_truth_host.py)


# ---- builders (shared with tests/test_antialias_gpu.py) --------------------------------------------------------------
def _cameras(eyes, width, height):
    B = eyes.shape[0]
    proj = camera_utils.perspective(torch.full((B,), width / height), torch.full((B,), 40.0),
                                    torch.full((B,), 0.01), torch.full((B,), 10.0))
    view = camera_utils.look_at(eyes, torch.zeros(B, 3), torch.tensor([[0.0, 1.0, 0.0]]).repeat(B, 1))
    return torch.matmul(proj, view)


def _cube_clip(eyes, width, height):
    vertices, triangles, _ = shapes.cube(2.0)
    triangles = torch.flip(triangles, [1]).contiguous()
    world = vertices.unsqueeze(0).repeat(eyes.shape[0], 1, 1)
    return camera_utils.transform_homogeneous(_cameras(eyes, width, height), world).contiguous(), triangles


CUBE_EYES = torch.tensor([[2.0, 3.0, 6.0], [-4.0, 1.0, 4.5], [0.3, -2.0, 5.0], [5.0, 0.5, -3.0]])


def _soup(seed, B=2, T=60, V=90):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(B, V, 2, generator=g) * 2.4 - 1.2
    w = torch.rand(B, V, 1, generator=g) + 0.5
    w[:, :3] = -0.3                                               # a triangle across the camera plane
    zz = torch.rand(B, V, 1, generator=g) * 1.6 - 0.8
    clip = torch.cat([xy * w, zz * w, w], 2).contiguous()
    tris = torch.randint(0, V, (T, 3), generator=g, dtype=torch.int32)
    strip = torch.arange(T // 2, dtype=torch.int32)
    tris[: T // 2] = torch.stack([strip, strip + 1, strip + 2], 1)   # a strip: neighbours share edges
    return clip, tris


def _square(W, H, left, right, bottom=None, top=None):
    """Two triangles forming a rectangle with its outline at the given positions in pixel units (pixel ix spans
    [ix, ix + 1]); without bottom / top it overshoots every row.  w = 1, so NDC = clip."""
    xl, xr = left / (W / 2) - 1.0, right / (W / 2) - 1.0
    yb, yt = (-2.0, 2.0) if bottom is None else (bottom / (H / 2) - 1.0, top / (H / 2) - 1.0)
    clip = torch.tensor([[[xl, yb, 0.0, 1.0], [xr, yb, 0.0, 1.0], [xr, yt, 0.0, 1.0], [xl, yt, 0.0, 1.0]]])
    return clip, torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)


def _pixel_triangle(W, H, corners, ws):
    """One triangle through the given pixel-unit corners, corner k at w = ws[k]."""
    rows = [[(x / (W / 2) - 1.0) * w, (y / (H / 2) - 1.0) * w, 0.25 * w, w] for (x, y), w in zip(corners, ws)]
    return torch.tensor([rows]), torch.tensor([[0, 1, 2]], dtype=torch.int32)


# ---- scenes ------------------------------------------------------------------------------------------------------------
RAGGED_SIZES = ((65, 47), (63, 5), (7, 3), (130, 6), (1, 9), (9, 1), (1, 1))
FULL_SWEEP = "ragged_65x47"                                      # the scene that runs every channel count
CHANNELS = (1, 2, 3, 4, 5, 7)


class Scene:
    def __init__(self, name, clip, tris, W, H, edit=None, C=4, unscaled=None, scale=1.0):
        self.name, self.W, self.H, self.edit, self.C = name, W, H, edit, C
        self.clip = np.ascontiguousarray(clip.numpy() if isinstance(clip, torch.Tensor) else clip, dtype=np.float32)
        self.tris = np.ascontiguousarray(tris.numpy() if isinstance(tris, torch.Tensor) else tris, dtype=np.int32).reshape(-1, 3)
        self.B, self.V, self.T = self.clip.shape[0], self.clip.shape[1], self.tris.shape[0]
        self.unscaled, self.scale = unscaled, scale
        self.seed = sum(map(ord, unscaled or name))                   # a scaled scene shares its inputs with the unscaled one

    def inputs(self, C=None, image_scale=1.0):
        """(image, dout) [B,H,W,C] float32, seeded by the scene's name and C; the image times image_scale (a float32
        product: the scaled image IS the input)."""
        C = C or self.C
        g = torch.Generator().manual_seed(self.seed * 16 + C)
        image = torch.rand(self.B, self.H, self.W, C, generator=g).numpy()
        dout = torch.randn(self.B, self.H, self.W, C, generator=g).numpy()
        return (image * np.float32(image_scale)).astype(np.float32), dout


def _roll(shift):
    def edit(sc, ids, bary, z, tris, opp):
        return np.roll(ids, shift, 2), np.roll(bary, shift, 2), np.roll(z, shift, 2), tris, opp
    return edit


def _poison(sc, ids, bary, z, tris, opp):
    """Ids outside [0, T) next to covered and next to uncovered pixels (also as the neighbour g of a covered pixel),
    one triangle naming vertex V, one opposite entry V + 3.  Seeded; the pixels are picked from the G-buffer given."""
    rng = np.random.default_rng(sc.seed)
    clean = ids
    ids, tris, opp = ids.copy(), tris.copy(), opp.copy()
    cov = (ids != 0) | (bary.sum(-1) >= 0.9)
    # the two triangles the most pixels of image 0 see: one loses a vertex, the other an entry of its topology
    seen = np.bincount(ids[0][cov[0]], minlength=sc.T)
    order = np.argsort(-seen, kind="stable")
    tris[order[0], 1] = sc.V
    opp[order[1], np.argmax(opp[order[1]] >= 0)] = sc.V + 3
    # the pairs of the clean G-buffer that blend a covered f into an uncovered g, poisoned triangles aside
    pairs, _ = ref.decide(clean, bary, z, sc.clip, sc.tris, ref.topology(sc.tris, sc.V))
    b, F = pairs["b"], clean[pairs["b"], pairs["fy"], pairs["fx"]]
    usable = np.nonzero(~cov[b, pairs["gy"], pairs["gx"]] & (F != order[0]) & (F != order[1]))[0]
    picks = usable[rng.permutation(len(usable))]
    near = np.zeros_like(cov)
    near[:, 1:-1, 1:-1] = True
    near &= ~cov & ~(np.roll(cov, 1, 2) | np.roll(cov, -1, 2) | np.roll(cov, 1, 1) | np.roll(cov, -1, 1))
    far = np.argwhere(near)                                          # uncovered among uncovered
    far = far[rng.permutation(len(far))]
    bad = (sc.T, sc.T + 7, -1, INT32_MIN)
    for i, v in enumerate(bad):
        p, q = picks[i], picks[len(bad) + i]
        ids[b[p], pairs["gy"][p], pairs["gx"][p]] = v               # as g of a covered pixel: the pair still blends
        ids[b[q], pairs["fy"][q], pairs["fx"][q]] = v               # as f next to an uncovered pixel: it no longer does
        ids[tuple(far[i])] = v
    return ids, bary, z, tris, opp


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith("ragged_"):
        W, H = (int(v) for v in name[7:].split("x"))
        clip, tris = _cube_clip(CUBE_EYES[:2], W, H)
        return Scene(name, clip, tris, W, H)
    if name == "seams_sphere":
        job = synthetic.sphere_job(2, 130, 10, 8)
        return Scene(name, job["clip"], job["triangles"], 130, 10)
    if name == "seams_soup":
        clip, tris = _soup(2)
        return Scene(name, clip, tris, 130, 10, C=3)
    if name == "long_edge":
        # bottom / top at t = 0.8: the pairs modify the UNCOVERED rows 1 and 6, whose wavefronts hold nothing else
        clip, tris = _square(128, 8, 2.3, 125.6, 1.7, 6.3)
        return Scene(name, clip, tris, 128, 8)
    if name == "spike":
        clip, tris = _pixel_triangle(9, 7, ((4.55, 3.9), (3.8, 3.1), (5.2, 3.1)), (0.8, 1.3, 1.1))
        return Scene(name, clip, tris, 9, 7, C=3)
    if name == "midpoint":
        clip, tris = _square(8, 4, 2.0, 5.0)
        return Scene(name, clip, tris, 8, 4)
    if name == "centre":
        clip, tris = _square(8, 4, 2.5, 5.5)
        return Scene(name, clip, tris, 8, 4)
    if name == "coplanar":
        a, _ = _pixel_triangle(16, 12, ((1.3, 1.2), (12.4, 2.1), (5.2, 10.7)), (1.0, 1.0, 1.0))
        b, _ = _pixel_triangle(16, 12, ((14.6, 10.4), (3.3, 8.2), (10.1, 0.8)), (1.0, 1.0, 1.0))
        return Scene(name, torch.cat([a, b], 1), torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32), 16, 12)
    if name in ("rolled_1", "rolled_2", "poisoned"):
        clip, tris = _cube_clip(CUBE_EYES[:2], 65, 47)
        return Scene(name, clip, tris, 65, 47, edit=_poison if name == "poisoned" else _roll(int(name[-1])))
    if name in SCALED:
        clip, tris = _soup(1)
        lam = SCALED[name]
        return Scene(name, clip * lam, tris, 67, 41, C=3, unscaled="scaled_1", scale=lam)
    if name == "no_triangles":
        return Scene(name, np.ones((2, 5, 4), np.float32), np.zeros((0, 3), np.int32), 70, 6)
    if name == "no_images":
        clip, tris = _cube_clip(CUBE_EYES[:1], 9, 7)
        return Scene(name, clip[:0], tris, 9, 7)
    raise KeyError(name)


SCALED = {"scaled_1": 1.0, "scaled_down": 2.0 ** -6, "scaled_up": 2.0 ** 5}
RAGGED = tuple("ragged_%dx%d" % s for s in RAGGED_SIZES)
SCENES = RAGGED + ("seams_sphere", "seams_soup", "long_edge", "spike", "midpoint", "centre", "coplanar", "rolled_1",
                   "rolled_2", "poisoned") + tuple(SCALED) + ("no_triangles", "no_images")
UNBLENDED = ("ragged_1x1", "midpoint", "no_triangles", "no_images")   # out is the image, dclip exactly zero
RASTERIZED = tuple(n for n in SCENES if n not in ("no_triangles", "no_images"))


def assemble(sc, ids, bary, z):
    """The G-buffer a rasterizer gave for (sc.clip, sc.tris) -> what antialias is called with: (ids, bary, z, tris, opp),
    host arrays, after the scene's edit."""
    opp = ref.topology(sc.tris, sc.V)
    ids, bary, z = (np.ascontiguousarray(a) for a in (ids, bary, z))
    if sc.edit is None:
        return ids, bary, z, sc.tris, opp
    return tuple(np.ascontiguousarray(a) for a in sc.edit(sc, ids, bary, z, sc.tris, opp))


def blank_gbuffer(sc):
    return (np.zeros((sc.B, sc.H, sc.W), np.int32), np.zeros((sc.B, sc.H, sc.W, 3), np.float32),
            np.zeros((sc.B, sc.H, sc.W), np.float32))


@functools.lru_cache(maxsize=None)
def host(name):
    """(scene, (ids, bary, z, tris, opp), pairs, mask) from the oracle's G-buffer."""
    import oracle
    sc = scene(name)
    raw = oracle.forward(sc.clip, sc.tris, sc.W, sc.H) if name in RASTERIZED else blank_gbuffer(sc)
    g = assemble(sc, *raw)
    pairs, mask = ref.decide(g[0], g[1], g[2], sc.clip, g[3], g[4])
    return sc, g, pairs, mask


class Truth:
    """The float64 truth of one scene's three outputs with their noise scales, and the float32 restatement's distance
    from it (r32: the largest |f32 - f64| / (2^-24 noise) over out, dimage and dclip)."""

    def __init__(self, sc, pairs, image, dout):
        self.out, self.n_out = ref.blend(image, pairs)
        self.dimage, self.n_dimage = ref.blend_backward(dout, pairs)
        self.dclip, self.n_dclip = ref.pair_gradients(image, dout, sc.clip, pairs)
        self.r32 = {"out": ref.r32_ratio(ref.blend(image, pairs, np.float32)[0], self.out, self.n_out),
                    "dimage": ref.r32_ratio(ref.blend_backward(dout, pairs, np.float32)[0], self.dimage, self.n_dimage),
                    "dclip": ref.r32_ratio(ref.pair_gradients(image, dout, sc.clip, pairs, np.float32)[0], self.dclip,
                                           self.n_dclip)}
        self.det_extra = det_quantisation(sc, pairs, image, dout)


# ---- what the wavefronts of k_aa_backward see ----------------------------------------------------------------------
TILE_W, TILE_H = 64, 4


def wave_of(pairs):
    """The wavefront (image, tile column, row) of the lane that commits each pair: its MODIFIED pixel's."""
    return pairs["b"], pairs["mx"] // TILE_W, pairs["my"]


def per_wave_vertex(pairs, V):
    """One key per (wavefront, vertex) a pair names, for both of its vertices: [2,n] int64."""
    b, tx, y = wave_of(pairs)
    wave = (b.astype(np.int64) * 4096 + tx) * 65536 + y
    return np.stack([(wave * V + pairs["va"]), (wave * V + pairs["vb"])]), wave


def det_quantisation(sc, pairs, image, dout):
    """Deterministic mode's own error per element of dclip [B,V,4], from csrc/det_fixed.h: a wavefront commits one
    sum per vertex and column, rounded to the nearest multiple of 2^-k (__float2ll_rn), k = 41 - e where the largest
    |per-wavefront sum| g = m 2^e, m in [0.5, 1): at most 2^(e - 42) per commit -> n_commits 2^-42 2^e.  g is taken
    from the float64 truth, a shade larger so that a float32 g just across a power of two is covered."""
    out = np.zeros(sc.clip.shape, np.float64)
    if len(pairs["b"]) == 0:
        return out
    p = ref.pair_terms(image, dout, sc.clip, pairs)
    keys, _ = per_wave_vertex(pairs, sc.V)
    uniq, inv = np.unique(keys.reshape(-1), return_inverse=True)
    sums = np.zeros((len(uniq), 3))
    np.add.at(sums, inv.reshape(-1), np.concatenate([p["ga"], p["gb"]]))
    g = float(np.abs(sums[np.isfinite(sums)]).max()) if np.isfinite(sums).any() else 0.0
    if g == 0.0:
        return out
    quantum = 2.0 ** (np.frexp(g * (1 + 2.0 ** -20))[1] - 42)
    vertex = uniq % sc.V
    image_of = uniq // sc.V // (4096 * 65536)
    commits = np.zeros(sc.clip.shape[:2])
    np.add.at(commits, (image_of, vertex), 1.0)
    out[..., 0] = out[..., 1] = out[..., 3] = (commits * quantum)
    return out


def regimes(sc, pairs, mask):
    """What a scene reaches, from the restatement's pairs alone -> dict of counts."""
    b, hor = pairs["b"], pairs["horizontal"]
    n = len(b)
    lo_x, lo_y = np.minimum(pairs["fx"], pairs["gx"]), np.minimum(pairs["fy"], pairs["gy"])
    out = {"pairs": n,
           "seam_x": int((hor & (lo_x % TILE_W == TILE_W - 1)).sum()),
           "seam_y": int((~hor & (lo_y % TILE_H == TILE_H - 1)).sum()),
           "mask15": int((mask == 15).sum()),
           "t0": int((pairs["t"] == 0).sum()), "t1": int((pairs["t"] == 1).sum()),
           "half": int(pairs["candidates"]["half"].sum()),
           "candidates": len(pairs["candidates"]["b"]),
           "equal_z_blended": int((pairs["candidates"]["equal_z"] & pairs["candidates"]["blended"]).sum()),
           "lane_repeat": 0, "wave_most_vertices": 0, "wave_two_vertices": 0}
    if n == 0:
        return out
    # a lane whose pairs share a vertex: the same key in several of its eight slots
    pixel = (b.astype(np.int64) * sc.H + pairs["my"]) * sc.W + pairs["mx"]
    slot = np.concatenate([pixel * sc.V + pairs["va"], pixel * sc.V + pairs["vb"]])
    out["lane_repeat"] = int((np.unique(slot, return_counts=True)[1] > 1).sum())
    keys, wave = per_wave_vertex(pairs, sc.V)
    for w in np.unique(wave):
        sel = wave == w
        distinct = len(np.unique(keys[:, sel]))
        out["wave_most_vertices"] = max(out["wave_most_vertices"], distinct)
        if distinct == 2:
            out["wave_two_vertices"] = max(out["wave_two_vertices"], int(sel.sum()))
    return out
