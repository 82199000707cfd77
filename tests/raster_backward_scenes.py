"""Scenes, float64 truth and per-element bound for mr_rasterize_backward (TEST INFRASTRUCTURE, no GPU needed).

Shared by tests/test_raster_backward_truth_host.py (the scenes reach the regimes they are built for, the reference
alone sits inside the rounding model) and tests/test_raster_backward_truth_gpu.py (the kernels against the truth).

Every scene is a seeded, pure function of its name.  The upstream gradient is dbary = N(0,1) / (H W) in float32, as
in backward_fuzz.  The G-buffer is the caller's: the oracle's on the host, the device's on the GPU (bit-identical;
tests/test_raster_gpu.py pins that).

  grid2     70 x 133, B = 2, a planar grid of 2-pixel quads (two triangles each) under two perspective tilts, the second
            also turned in the image plane: every pixel covered; thousands of distinct triangles per 64 x 128 region (the
            deterministic kernel's 512-slot LDS hash saturates), far more than 16 per 4-row strip (the lane kernel's merge
            table overflows), every lane changes triangle in the same row (dense flush); a 6-pixel second column strip;
            133 rows = a 1-row tail for 4-row strips and a 5-row tail for 16-row strips (odd trip counts of the
            two-rows-ahead loop)
  grid24    the same grid with 24-pixel quads at 130 x 67: three column strips, the last 2 pixels wide; the diagonal (and
            turned) edges finish a few lanes per row (sparse flush)
  soup_*    three soups of the stand-alone fuzzer's recipe (slivers, repeated and degenerate triangles), B = 1..3, at
            70 x 37, 180 x 129 and 65 x 5
  sphere    synthetic.sphere_job(2, 128, 96): sub-pixel triangles at the poles
  tiny_*    one soup at 1 x 1, 7 x 3 and 64 x 4: H smaller than the strip, W <= 64
  auto16    one soup at B = 128, W = 8, H = 1024: 128 * 1 * 64 = 8192 strips of 16 rows, so the automatic rule of
            lanes_rows_per_wave keeps 16 rows with nothing forced
  edited    the 70 x 37 soup's G-buffer with poisoned pixels (edit_gbuffer)

THE BOUND (per element; calibrated by the oracle, never by a kernel).  With d, n = truth64.raster_pullback (gradient
and noise scale: the sum of |terms| in the reference's evaluation order) and o = oracle.backward (the C port, bit for
bit the reference):

    u = 2^-24 n + 1e-7,   r = max |o - d| / u,   K_scene = min(64, max(4, 8 r)),   |kernel - d| <= K_scene u

  8   the margin soft_truth.K, the camera and the normals truths use: it covers another summation order
  4   the floor: the kernels multiply by a rounded reciprocal of |det| where the reference divides (raster_backward.hip's
      header: <= 1.5 ulp per partial = 3 units of 2^-24 on a partial without cancellation), which the oracle's own
      error does not contain
  64  the cap: backward_fuzz.K_ROUNDING
"""
import hashlib

import numpy as np

import oracle
from oracle import truth64

FLOOR = 1e-7
MARGIN, K_MIN, K_MAX = 8.0, 4.0, 64.0
CUTOFF = np.float32(0.9)           # rasterize_triangles.cpp:13
DET_HEADROOM = 2.0 ** 20           # per-pixel partial / max |dbary| a scene may reach and still run in deterministic mode
DET_QUANTUM = 2.0 ** -41           # rounding of one fixed-point conversion, in units of max |dbary| (det_fixed.h)
RUN_ROWS, RUN_REGION_H = 32, 128   # k_accumulate_runs: rows per wavefront, rows per workgroup (run_accum.h)


class Scene:
    def __init__(self, name, clip, tris, W, H, seed):
        self.name, self.W, self.H, self.seed = name, int(W), int(H), int(seed)
        self.clip = np.ascontiguousarray(clip, dtype=np.float32)
        self.tris = np.ascontiguousarray(tris, dtype=np.int32)
        self.B, self.V, self.T = self.clip.shape[0], self.clip.shape[1], self.tris.shape[0]

    def dbary(self):
        rng = np.random.default_rng(1000 + self.seed)
        return (rng.normal(size=(self.B, self.H, self.W, 3)) / (self.H * self.W)).astype(np.float32)


def _grid(name, W, H, quad, tilts, seed):
    """Planar grid of `quad`-pixel squares, two triangles each, reaching beyond the frame on every side; image b under
    tilts[b] = (a, b, angle): w = 1 + a x + b y over the NDC position (a perspective tilt) after a turn by `angle`
    about the image centre."""
    margin = int(np.ceil(8.0 / quad))
    nx, ny = int(np.ceil(W / quad)) + 2 * margin, int(np.ceil(H / quad)) + 2 * margin
    ix, iy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    px = (ix.reshape(-1) - margin) * float(quad) + 0.37      # no pixel centre on an edge or a diagonal
    py = (iy.reshape(-1) - margin) * float(quad) + 0.21
    at = lambda i, j: j * (nx + 1) + i
    tris = []
    for j in range(ny):
        for i in range(nx):
            tris.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
            tris.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
    clip = np.zeros((len(tilts), px.size, 4))
    for b, (ta, tb, angle) in enumerate(tilts):
        cx, cy = px - W / 2.0, py - H / 2.0
        rx, ry = np.cos(angle) * cx - np.sin(angle) * cy, np.sin(angle) * cx + np.cos(angle) * cy
        xn, yn = 2.0 * rx / W, 2.0 * ry / H
        w = 1.0 + ta * xn + tb * yn
        assert w.min() > 0.2
        clip[b] = np.stack([xn * w, yn * w, 0.1 * w, w], 1)
    return Scene(name, clip, np.array(tris), W, H, seed)


def _soup(name, W, H, B, V, T, scale, seed):
    """tests/fuzz_raster_backward_gpu.py's recipe: vertices anywhere in front of the eye, triangles drawn with
    repetition (repeated, degenerate and sliver triangles come by themselves)."""
    rng = np.random.default_rng(seed)
    clip = (rng.normal(size=(B, V, 4)) * [scale, scale, 1.0, 1.0]).astype(np.float32)
    clip[..., 3] = np.abs(clip[..., 3]) + 0.2
    tris = rng.integers(0, V, size=(T, 3)).astype(np.int32)
    return Scene(name, clip, tris, W, H, seed)


def _sphere(name):
    from pytorch_mesh_renderer_amd.common import synthetic
    job = synthetic.sphere_job(2, 128, 96)
    return Scene(name, job["clip"].numpy(), job["triangles"].numpy(), 128, 96, 7)


TILTS = ((0.2, -0.12, 0.0), (-0.15, 0.2, 0.06))
_BUILDERS = {
    "grid2": lambda n: _grid(n, 70, 133, 2, TILTS, 1),
    "grid24": lambda n: _grid(n, 130, 67, 24, TILTS, 2),
    "soup_70x37": lambda n: _soup(n, 70, 37, 2, 60, 300, 1.0, 11),
    "soup_180x129": lambda n: _soup(n, 180, 129, 3, 150, 1200, 2.0, 12),
    "soup_65x5": lambda n: _soup(n, 65, 5, 1, 20, 40, 0.3, 13),
    "sphere": _sphere,
    "tiny_1x1": lambda n: _soup(n, 1, 1, 2, 12, 30, 1.0, 21),
    "tiny_7x3": lambda n: _soup(n, 7, 3, 2, 12, 30, 1.0, 21),
    "tiny_64x4": lambda n: _soup(n, 64, 4, 2, 12, 30, 1.0, 21),
    "auto16": lambda n: _soup(n, 8, 1024, 128, 40, 80, 1.0, 31),
}
SCENES = tuple(_BUILDERS)
# the scenes that also run in deterministic mode: the host module asserts the headroom condition for each of them
DET_SCENES = ("grid2", "grid24", "sphere", "tiny_1x1", "tiny_7x3", "tiny_64x4", "soup_70x37")
_scene_cache, _truth_cache = {}, {}


def scene(name):
    if name not in _scene_cache:
        _scene_cache[name] = _BUILDERS[name](name)
    return _scene_cache[name]


def oracle_gbuffer(sc):
    ids, bary, _ = oracle.forward(sc.clip, sc.tris, sc.W, sc.H, threads=min(8, oracle.max_threads()))
    return ids, bary


def valid_pixels(ids, bary, T):
    """RasterGradFn::prepare(): the pixels a kernel processes -- an id inside [0, T), and not (id 0 with a binary32
    barycentric sum (b0 + b1) + b2 below 0.9)."""
    ids = np.asarray(ids)
    b = np.asarray(bary, dtype=np.float32)
    s = (b[..., 0] + b[..., 1]) + b[..., 2]
    return (ids >= 0) & (ids < T) & ~((ids == 0) & (s < CUTOFF))


class Truth:
    """d, n: truth64.raster_pullback; o: the oracle; u, r, K: module docstring; max_partial, gmax: the deterministic
    mode's headroom condition; finite: where d is finite (a degenerate triangle that owns a pixel has none)."""

    def __init__(self, sc, tris, ids, bary, dbary):
        stats = {}
        self.d, self.n = truth64.raster_pullback(sc.clip, tris, ids, bary, dbary.astype(np.float64), stats=stats)
        self.o = oracle.backward(dbary, sc.clip, tris, ids, bary).astype(np.float64)
        self.u = truth64.U32 * self.n + FLOOR
        self.finite = np.isfinite(self.d) & np.isfinite(self.u)
        self.r = ratio(self.o, self)
        self.K = min(K_MAX, max(K_MIN, MARGIN * self.r))
        self.max_partial = stats.get("max_partial", 0.0)
        self.gmax = float(np.abs(dbary).max())

    def det_headroom_ok(self):
        return self.max_partial < DET_HEADROOM * self.gmax


def ratio(got, truth):
    """max over the elements of |got - d| / u (a kernel passes with ratio <= K_scene).  NaN / inf in `got` where the
    truth is finite count as infinite."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - truth.d)
    err = np.where(np.isfinite(got), err, np.inf)
    m = truth.finite
    return float((err[m] / truth.u[m]).max()) if m.any() else 0.0


def relative_to_largest(got, truth):
    """Per image, max |got - d| / max |d| (for the record only)."""
    got = np.asarray(got, dtype=np.float64)
    out = []
    for b in range(got.shape[0]):
        m = truth.finite[b]
        top = float(np.abs(truth.d[b][m]).max()) if m.any() else 0.0
        out.append(float(np.abs(got[b] - truth.d[b])[m].max()) / top if top > 0 else 0.0)
    return out


def truth(sc, ids, bary, tris=None, key=None):
    """The scene's Truth on the given G-buffer, computed once per (scene, G-buffer bits) and shared."""
    tris = sc.tris if tris is None else tris
    h = hashlib.sha256(np.ascontiguousarray(ids).tobytes())
    h.update(np.ascontiguousarray(bary).tobytes())
    key = (key or sc.name, h.hexdigest())
    if key not in _truth_cache:
        _truth_cache[key] = Truth(sc, tris, ids, bary, sc.dbary())
    return _truth_cache[key]


# ---- the edited G-buffer -----------------------------------------------------------------------------------------

def edit_gbuffer(sc, ids, bary):
    """Poison the scene's G-buffer (soup_70x37's) -> dict(tris: the triangles with one appended; ids_p, bary_p: the
    poisoned buffer; ids_c, bary_c: the clean one; poisoned: mask; ids_s, ids_sc: see below).

    The appended triangle T names vertex index V (k_bwd_setup zeroes its record, k_bwd_scatter skips the corner).
    Poisoned pixels, 40 of each: ids T + 1 (the first foreign one), -1 and 2^30 (prepare(): foreign id), id T (the
    appended triangle), id 0 with a barycentric sum just below 0.9 (cpp:162: background).  All of them count as
    background for the truth: in the clean buffer they are id 0 with zero barycentrics.  40 further pixels get id 0 with
    a sum just ABOVE 0.9: those stay in both buffers -- they belong to triangle 0 and contribute.

    WHERE the appended triangle's pixels sit.  A pixel the kernels skip (foreign id, background) leaves the run of its
    column open; a pixel of ANY triangle -- also one whose record is all zeros -- ends it, and the two halves of the run
    are then rounded separately: same terms, another association of the binary32 sum inside the run.  So that `exactly
    nothing` can be asked bit for bit, the 40 pixels of triangle T sit on the first row of a 32-row segment of the
    deterministic kernel (rows 0 and 32), where no run is open.  ids_s is the poisoned buffer with 40 MORE pixels of
    triangle T scattered anywhere (ids_sc: the same set to background): there the two results may differ in the
    association of a few sums, and only that (tests/test_raster_backward_truth_gpu.py)."""
    rng = np.random.default_rng(77)
    V, T = sc.V, sc.T
    B, H, W = ids.shape
    tris = np.concatenate([sc.tris, np.array([[V, 0, 1]], np.int32)], 0)
    ids_p, bary_p = ids.copy(), bary.copy()
    n = ids.size
    rows = (np.arange(n) // W) % H
    first_rows = np.flatnonzero(rows % RUN_ROWS == 0)
    dead = rng.choice(first_rows, size=40, replace=False)
    rest = np.setdiff1d(np.arange(n), dead)
    picks = rng.choice(rest, size=6 * 40, replace=False).reshape(6, -1)
    flat_ids, flat_bary = ids_p.reshape(-1), bary_p.reshape(-1, 3)
    for k, bad in enumerate((T + 1, -1, 2 ** 30)):
        flat_ids[picks[k]] = bad
    flat_ids[dead] = T
    flat_ids[picks[3]] = 0
    flat_bary[picks[3]] = np.array([0.3, 0.3, 0.2999], np.float32)      # 0.8999: background
    flat_ids[picks[4]] = 0
    flat_bary[picks[4]] = np.array([0.3, 0.3, 0.3001], np.float32)      # 0.9001: triangle 0
    poisoned = np.zeros(n, bool)
    poisoned[picks[:4].reshape(-1)] = True
    poisoned[dead] = True
    ids_c, bary_c = ids_p.copy(), bary_p.copy()
    ids_c.reshape(-1)[poisoned] = 0
    bary_c.reshape(-1, 3)[poisoned] = 0.0
    ids_s, ids_sc = ids_p.copy(), ids_p.copy()
    ids_s.reshape(-1)[picks[5]] = T
    ids_sc.reshape(-1)[picks[5]] = 0
    bary_sc = bary_p.copy()
    bary_sc.reshape(-1, 3)[picks[5]] = 0.0
    return dict(tris=tris, ids_p=ids_p, bary_p=bary_p, ids_c=ids_c, bary_c=bary_c, poisoned=poisoned.reshape(ids.shape),
                ids_s=ids_s, ids_sc=ids_sc, bary_sc=bary_sc)


# ---- host emulation of the kernels' bookkeeping (which regimes does a G-buffer reach?) -----------------------------

def lane_regimes(ids, bary, T, rows):
    """k_accumulate_lanes with `rows`-row strips on this G-buffer -> dict:
      finished_per_row   sorted distinct counts of lanes that finish a run in one row of one strip (flush(): >= 20 takes
                         the dense pass, 1..19 the sparse one; the strip's end, where every open lane finishes, is not
                         counted)
      max_distinct       most distinct triangles in one strip (> 16: the merge table's full-table flush)
      strip_rows         distinct trip counts of the row loop
      last_strip_width   pixels in the last column strip"""
    ids = np.asarray(ids)
    valid = valid_pixels(ids, bary, T)
    B, H, W = ids.shape
    counts, most, trips = set(), 0, set()
    for b in range(B):
        for y0 in range(0, H, rows):
            y1 = min(y0 + rows, H)
            trips.add(y1 - y0)
            for x0 in range(0, W, 64):
                t, v = ids[b, y0:y1, x0:x0 + 64], valid[b, y0:y1, x0:x0 + 64]
                most = max(most, int(np.unique(t[v]).size))
                run = np.full(t.shape[1], -1, np.int64)
                for y in range(t.shape[0]):
                    fin = v[y] & (run >= 0) & (t[y] != run)
                    if fin.any():
                        counts.add(int(fin.sum()))
                    run = np.where(v[y], t[y], run)
    return {"finished_per_row": sorted(counts), "max_distinct": most, "strip_rows": sorted(trips),
            "last_strip_width": W - 64 * ((W - 1) // 64)}


def run_regimes(ids, bary, tris, V):
    """k_accumulate_runs (the deterministic mode's kernel) on this G-buffer -> (most distinct triangles in one 64 x 128
    region -- beyond 512 the LDS hash is full and runs go straight to memory --, runs feeding each vertex [B,V]: every run
    is ONE fixed-point conversion per sum, so a vertex's quantisation error is at most that many half quanta)."""
    ids = np.asarray(ids)
    tris = np.asarray(tris)
    T = tris.shape[0]
    valid = valid_pixels(ids, bary, T)
    B, H, W = ids.shape
    most = 0
    feeding = np.zeros((B, V + 1), np.int64)     # (column V: the appended triangle's foreign corner, dropped)
    for b in range(B):
        for y0 in range(0, H, RUN_REGION_H):
            for x0 in range(0, W, 64):
                t, v = ids[b, y0:y0 + RUN_REGION_H, x0:x0 + 64], valid[b, y0:y0 + RUN_REGION_H, x0:x0 + 64]
                most = max(most, int(np.unique(t[v]).size))
        for y0 in range(0, H, RUN_ROWS):
            run = np.full(W, -1, np.int64)
            for y in range(y0, min(y0 + RUN_ROWS, H)):
                start = valid[b, y] & (ids[b, y] != run)
                for j in range(3):
                    np.add.at(feeding[b], np.minimum(tris[ids[b, y][start], j], V), 1)
                run = np.where(valid[b, y], ids[b, y], run)
    return most, feeding[:, :V]
