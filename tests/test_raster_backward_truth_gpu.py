"""mr_rasterize_backward against the float64 truth in every regime of its two pixel passes (GPU).

The scenes, the truth and the per-element bound |kernel - d| <= K_scene (2^-24 n + 1e-7) are those of
tests/raster_backward_scenes.py (K_scene = min(64, max(4, 8 r)), r the ORACLE's distance from the truth in the same
unit: the bound is calibrated by the reference, never by a kernel); tests/test_raster_backward_truth_host.py shows on
the CPU that each scene reaches the regime it is built for.

  float path          k_accumulate_lanes<RasterLanesFn> (the pipelined two-rows-ahead row loop) under the automatic
                      strip height and under forced 4, 8 and 16 rows (mr_debug_set_lanes_rows), every scene
  deterministic mode  k_accumulate_runs<RasterGradFn, true> (512-slot LDS hash, fixed point): same bound, two calls
                      bit-identical, no NaN; the quantisation term (runs feeding a vertex) 2^-41 max|dbary| is asserted
                      to be below the bound's floor, not assumed
  edited G-buffer     foreign ids, a triangle naming vertex V, id 0 on either side of the 0.9 cut-off: on both paths
                      inside the bound of the truth that counts them as background, and in deterministic mode
                      bit-equal to the buffer with those pixels set to background (the zero-record triangle's pixels
                      where no run is open; anywhere else they still add exactly zero but split the run they
                      interrupt: 8 elements move by 2.3e-10 at most -- raster_backward_scenes.edit_gbuffer)

MEASURED (MI355X; `worst` = the kernel's largest |kernel - d| / u over the four strip heights, to be held against
K_scene; the last two columns for the record only: max |x - d| / max |d| over the images, kernel and oracle):

    scene          r       K_scene   lanes: worst of auto / 4 / 8 / 16   deterministic   kernel      oracle
    grid2          0.097   4.0       0.097                               0.097           2.7e-05     2.7e-05
    grid24         0.041   4.0       0.008                               0.005           2.2e-07     1.5e-06
    soup_70x37     0.076   4.0       0.076                               0.070           9.6e-07     1.0e-06
    soup_180x129   0.025   4.0       0.022                               -               9.7e-07     1.9e-06
    soup_65x5      0.037   4.0       0.031                               -               4.4e-07     5.0e-07
    sphere         0.091   4.0       0.090                               0.090           5.2e-05     5.1e-05
    tiny_1x1       0.138   4.0       0.080                               0.080           1.0e-07     1.0e-07
    tiny_7x3       0.149   4.0       0.077                               0.077           2.8e-07     2.8e-07
    tiny_64x4      0.079   4.0       0.025                               0.025           1.5e-07     4.8e-07
    auto16         0.318   4.0       0.318                               -               2.2e-05     2.2e-05
    edited         0.076   4.0       0.076                               0.076           9.6e-07     9.6e-07
    200 fuzz soups <= 0.303  4.0     0.31                                0.32            (backward_fuzz.raster_trial, seed 505)

No scene needs more than the floor K_scene = 4; the kernels sit where the oracle sits (the per-pixel arithmetic is the
reference's, only the order of the sum over pixels differs), 12 times inside the bound at the worst.

MUTATIONS (each built into a copy of the library, arithmetic only; `ratio` as above on the first failing case):

    mutation                                          new tests that fail (worst |kernel - d| / u; K_scene = 4)                older tests
    (a) close_segment drops sum2                      float path: grid24 16357, the three soups 5049..8495, tiny_64x4         19 of the 58 of
        (lane kernel, dense pass)                     130646, edited 8579; raster row of the random soups 4041 x its bound                test_raster_gpu
    (b) open_segment on a hit starts from merged = 0  float path: every scene but tiny_1x1, 4720 (grid2) .. 563700 (tiny_7x3);  14 of 58
                                                      edited 49273; raster row 8422 x its bound
    (c) second row of the pipelined pair runs only    float path: every scene but tiny_1x1 / tiny_7x3, 9508 .. 156609          20 of 58
        `if (y + 2 < y_end)`: a tail row skipped      (soup_65x5 at 4-row strips only: its 5 rows are ONE odd strip at 8 and
                                                      16); edited 62432; raster row 3850 x its bound
    (d) run_flush drops the run when the LDS hash     deterministic mode on grid2 and sphere: two calls differ (which runs    none: all 58
        is saturated                                  are dropped depends on the order the table fills); all else passes      pass
    (e) prepare() treats every id 0 as background     float path: soup_180x129 1272, auto16 48002; edited 6429 (both paths);   11 of 58
                                                      raster row 617 x its bound on both kernels
"""
import numpy as np
import pytest
import torch

import raster_backward_scenes as rs
from pytorch_mesh_renderer_amd import _native

pytestmark = pytest.mark.gpu

_device_cache = {}


def on_device(name, device):
    """The scene's inputs on the device and the DEVICE's G-buffer (also as host arrays), once per scene."""
    if name not in _device_cache:
        sc = rs.scene(name)
        clip, tris, dbary = (torch.from_numpy(a).to(device) for a in (sc.clip, sc.tris, sc.dbary()))
        ids, bary, _ = _native.rasterize_forward(clip, tris, sc.W, sc.H)
        _device_cache[name] = (sc, clip, tris, dbary, ids, bary, ids.cpu().numpy(), bary.cpu().numpy())
    return _device_cache[name]


def automatic_rows(B, W, H):
    """lanes_rows_per_wave (run_accum.h) for RasterLanesFn."""
    rows = 16
    while rows > 4 and B * -(-W // 64) * -(-H // rows) < 8192:
        rows //= 2
    return rows


def lanes_at_every_height(dbary, clip, tris, ids, bary):
    """The float path under the automatic strip height and under forced 4, 8, 16 -> {rows asked: dclip (host)}."""
    B, H, W = ids.shape
    out = {}
    try:
        for rows in (0, 4, 8, 16):
            _native.debug_set_lanes_rows(rows)
            got = _native.rasterize_backward(dbary, clip, tris, ids, bary)
            ran, used = _native.debug_last_accumulate_kernel(), _native.debug_last_lanes_rows()
            assert ran.startswith("RasterLanesFn"), ran
            assert used == (rows or automatic_rows(B, W, H)), (rows, used)
            out[rows] = got.cpu().numpy()
    finally:
        _native.debug_set_lanes_rows(0)
    return out


def deterministic_twice(dbary, clip, tris, ids, bary):
    before = _native.set_deterministic(True)
    try:
        a = _native.rasterize_backward(dbary, clip, tris, ids, bary)
        ran = _native.debug_last_accumulate_kernel()
        b = _native.rasterize_backward(dbary, clip, tris, ids, bary)
    finally:
        _native.set_deterministic(before)
    assert ran.startswith("RasterGradFn"), ran
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert not np.isnan(a).any() and np.isfinite(a).all()
    assert a.tobytes() == b.tobytes(), "two deterministic calls differ"
    return a


def record(name, path, t, got):
    worst = rs.ratio(got, t)
    rel, rel_o = rs.relative_to_largest(got, t), rs.relative_to_largest(t.o, t)
    print("RBT | %-13s | %-14s | r %.3f | K_scene %4.1f | worst %6.3f | kernel %.1e | oracle %.1e" % (
        name, path, t.r, t.K, worst, max(rel), max(rel_o)))
    per_image = lambda v: " ".join("%.1e" % x for x in v[:4]) + (" ... (%d images)" % len(v) if len(v) > 4 else "")
    print("    per image, max |x - d| / max |d|: kernel %s | oracle %s" % (per_image(rel), per_image(rel_o)))
    return worst


def test_lanes_rows_hook_validates_and_defaults_to_automatic(device):
    L = _native.lib()
    try:
        for bad in (-1, 1, 2, 5, 12, 32, 64):
            assert L.mr_debug_set_lanes_rows(bad) == _native.MR_EINVAL
        for ok in (4, 8, 16, 0):
            assert L.mr_debug_set_lanes_rows(ok) == _native.MR_OK
    finally:
        L.mr_debug_set_lanes_rows(0)
    sc, clip, tris, dbary, ids, bary, _, _ = on_device("grid2", device)
    _native.rasterize_backward(dbary, clip, tris, ids, bary)
    assert _native.debug_last_lanes_rows() == 4            # a small image: the automatic rule halves 16 -> 8 -> 4
    sc, clip, tris, dbary, ids, bary, _, _ = on_device("auto16", device)
    _native.rasterize_backward(dbary, clip, tris, ids, bary)
    assert _native.debug_last_lanes_rows() == 16           # 128 * 1 * 64 = 8192 strips: nothing to halve for


@pytest.mark.parametrize("name", rs.SCENES)
def test_float_path_at_every_strip_height(device, name):
    sc, clip, tris, dbary, ids, bary, ids_h, bary_h = on_device(name, device)
    t = rs.truth(sc, ids_h, bary_h)
    got = lanes_at_every_height(dbary, clip, tris, ids, bary)
    worst = {rows: record(name, "lanes %s" % (rows or "auto"), t, g) for rows, g in got.items()}
    for g in got.values():
        assert np.all(g[..., 2] == 0.0)
    assert max(worst.values()) <= t.K, "%s: %s times the unit, K_scene %.1f (r %.3f)" % (name, worst, t.K, t.r)


@pytest.mark.parametrize("name", rs.DET_SCENES)
def test_deterministic_mode(device, name):
    sc, clip, tris, dbary, ids, bary, ids_h, bary_h = on_device(name, device)
    t = rs.truth(sc, ids_h, bary_h)
    assert t.det_headroom_ok() and t.finite.all(), (t.max_partial, t.gmax)     # then a NaN is a failure, not the overflow policy
    most, feeding = rs.run_regimes(ids_h, bary_h, sc.tris, sc.V)
    quant = feeding.max() * rs.DET_QUANTUM * t.gmax
    print("RBT | %-13s | most triangles per 64x128 region %d, most runs feeding a vertex %d: quantisation <= %.1e" % (
        name, most, feeding.max(), quant))
    assert quant < rs.FLOOR
    if name == "grid2":
        assert most > 512                                    # the saturated table: runs go straight to memory
    got = deterministic_twice(dbary, clip, tris, ids, bary)
    worst = record(name, "deterministic", t, got)
    assert np.all(got[..., 2] == 0.0)
    assert worst <= t.K, "%s: %.2f times the unit, K_scene %.1f" % (name, worst, t.K)


def test_edited_gbuffer_contributes_exactly_nothing(device):
    sc, clip, _, dbary, _, _, ids_h, bary_h = on_device("soup_70x37", device)
    e = rs.edit_gbuffer(sc, ids_h, bary_h)
    tris_h, ids_p, bary_p, ids_c, bary_c = (e[k] for k in ("tris", "ids_p", "bary_p", "ids_c", "bary_c"))
    t = rs.truth(sc, ids_c, bary_c, key="edited")
    assert t.det_headroom_ok() and t.finite.all()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    tris, ids_pd, bary_pd, ids_cd, bary_cd = map(dev, (tris_h, ids_p, bary_p, ids_c, bary_c))
    got = lanes_at_every_height(dbary, clip, tris, ids_pd, bary_pd)
    worst = {rows: record("edited", "lanes %s" % (rows or "auto"), t, g) for rows, g in got.items()}
    assert max(worst.values()) <= t.K, (worst, t.K)
    det_p = deterministic_twice(dbary, clip, tris, ids_pd, bary_pd)
    det_c = deterministic_twice(dbary, clip, tris, ids_cd, bary_cd)
    assert record("edited", "deterministic", t, det_p) <= t.K
    assert det_p.tobytes() == det_c.tobytes(), "poisoned pixels moved %d elements, by up to %.3e" % (
        int((det_p != det_c).sum()), float(np.abs(det_p - det_c).max()))
    # ... and the float path sees the same pixels: clean buffer, same bound
    clean = lanes_at_every_height(dbary, clip, tris, ids_cd, bary_cd)
    assert max(rs.ratio(g, t) for g in clean.values()) <= t.K
    # Pixels of the zero-record triangle ANYWHERE (edit_gbuffer: ids_s) still add exactly zero, but each one ends the run
    # it interrupts, and the halves round separately: against the same pixels as background the deterministic result
    # may move in the last bits of a few sums (measured: 7 elements, by 5.8e-11 at most, gradients of 2e-2) -- held to
    # one unit of the bound here, and printed
    det_s = deterministic_twice(dbary, clip, tris, dev(e["ids_s"]), bary_pd)
    det_sc = deterministic_twice(dbary, clip, tris, dev(e["ids_sc"]), dev(e["bary_sc"]))
    moved = np.abs(det_s.astype(np.float64) - det_sc)
    print("RBT | edited        | zero-record pixels inside runs: %d elements move, by %.1e at most (unit >= %.0e)" % (
        int((moved > 0).sum()), float(moved.max()), rs.FLOOR))
    assert np.all(moved <= t.u)
