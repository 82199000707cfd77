"""The scenes of tests/raster_backward_scenes.py are fit to judge mr_rasterize_backward by (no GPU needed): each one
reaches the regime of the pixel passes it is built for -- checked on the oracle's G-buffer by a host emulation of the
kernels' bookkeeping --, the reference alone (the oracle) sits well inside the rounding model (r <= 1, so K_scene is its
floor of 4 unless a scene says otherwise), and the scenes that run in deterministic mode stay inside its fixed-point
range, so that a NaN there is a failure and not the overflow policy.

MEASURED on one x86 host (the oracle is sequential, so r does not depend on the host's thread count):

    scene          r       K_scene   max partial / max|dbary|   most runs feeding a vertex   quantisation <=
    grid2          0.097   4.0       2^5.7                      12                           2.4e-15
    grid24         0.041   4.0       2^1.8                      197                          4.8e-14
    soup_70x37     0.076   4.0       2^3.3                      327                          2.4e-13
    soup_180x129   0.025   4.0
    soup_65x5      0.037   4.0
    sphere         0.091   4.0       2^5.9                      54                           8.4e-15
    tiny_1x1       0.138   4.0       2^-0.4                     1                            9.0e-13
    tiny_7x3       0.149   4.0       2^0.2                      10                           6.0e-13
    tiny_64x4      0.079   4.0       2^0.6                      115                          7.6e-13
    auto16         0.318   4.0
    edited         0.076   4.0

    grid2: 4127 distinct triangles in the first 64 x 128 region (> 512); per strip of 4 / 8 / 16 rows up to 164 / 289 / 537
    (> 16); lanes finishing in one row: 2..6, 32, 45..56, 64.  grid24: at most 11 / 13 / 14 per strip; 1..20 lanes per row.
"""
import numpy as np
import pytest

import raster_backward_scenes as rs

_gbuffers = {}


def gbuffer(name):
    if name not in _gbuffers:
        _gbuffers[name] = rs.oracle_gbuffer(rs.scene(name))
    return _gbuffers[name]


def scene_truth(name):
    sc = rs.scene(name)
    ids, bary = gbuffer(name)
    return sc, ids, bary, rs.truth(sc, ids, bary)


@pytest.mark.parametrize("name", rs.SCENES)
def test_scenes_are_seeded_and_pure(name):
    a, b = rs._BUILDERS[name](name), rs._BUILDERS[name](name)
    assert a.clip.tobytes() == b.clip.tobytes() and a.tris.tobytes() == b.tris.tobytes()
    assert a.dbary().tobytes() == b.dbary().tobytes() and a.dbary().dtype == np.float32
    assert a.clip.dtype == np.float32 and a.tris.dtype == np.int32 and a.clip.shape == (a.B, a.V, 4)
    # N(0,1) / (H W): the largest of H W 3 B draws is a few sigma
    assert 0 < float(np.abs(a.dbary()).max()) * a.H * a.W < 7.0


def test_grid2_reaches_the_saturated_hash_the_full_merge_table_and_the_dense_flush():
    sc, ids, bary, _ = scene_truth("grid2")
    assert (sc.W, sc.H, sc.B) == (70, 133, 2)
    valid = rs.valid_pixels(ids, bary, sc.T)
    assert valid.all(), "every pixel is covered"
    assert bool((bary.sum(-1) > 0.99).all())
    assert not np.array_equal(ids[0], ids[1]) or not np.array_equal(bary[0], bary[1])   # two different tilts
    most_region, _ = rs.run_regimes(ids, bary, sc.tris, sc.V)
    assert most_region > 4000 > 512, most_region           # the 512-slot table saturates (4212 under the first tilt)
    for rows in (4, 8, 16):
        g = rs.lane_regimes(ids, bary, sc.T, rows)
        print("grid2, %2d-row strips: %s" % (rows, g))
        assert g["max_distinct"] > 16                       # the merge table's full-table flush (171 at 4 rows)
        assert g["finished_per_row"][-1] == 64              # all 64 lanes change triangle in the same row
        assert min(c for c in g["finished_per_row"] if c >= 20) >= 20
        assert g["last_strip_width"] == 6
    assert rs.lane_regimes(ids, bary, sc.T, 4)["strip_rows"] == [1, 4]      # 133 = 33 * 4 + 1
    assert rs.lane_regimes(ids, bary, sc.T, 8)["strip_rows"] == [5, 8]      # odd trip counts of the pipelined loop
    assert rs.lane_regimes(ids, bary, sc.T, 16)["strip_rows"] == [5, 16]


def test_grid24_reaches_the_sparse_flush_in_three_column_strips():
    sc, ids, bary, _ = scene_truth("grid24")
    assert (sc.W, sc.H, sc.B) == (130, 67, 2)
    assert rs.valid_pixels(ids, bary, sc.T).all()
    for rows in (4, 8, 16):
        g = rs.lane_regimes(ids, bary, sc.T, rows)
        print("grid24, %2d-row strips: %s" % (rows, g))
        assert g["last_strip_width"] == 2 and -(-sc.W // 64) == 3
        sparse = [c for c in g["finished_per_row"] if 1 <= c <= 19]
        assert len(sparse) >= 3, g                          # a few lanes per row, more than one count
        assert g["strip_rows"] == [67 % rows, rows]
    # under the first tilt (axis-parallel) the sparse pass is all there is but for the quads' horizontal edges
    g0 = rs.lane_regimes(ids[:1], bary[:1], sc.T, 16)
    assert g0["max_distinct"] <= 16, g0


@pytest.mark.parametrize("name", ["soup_70x37", "soup_180x129", "soup_65x5"])
def test_soups_hold_repeated_degenerate_and_sliver_triangles(name):
    sc, ids, bary, t = scene_truth(name)
    assert 1 <= sc.B <= 3
    srt = np.sort(sc.tris, 1)
    assert (srt[:, 0] == srt[:, 1]).any() or (srt[:, 1] == srt[:, 2]).any(), "a degenerate triangle"
    valid = rs.valid_pixels(ids, bary, sc.T)
    cover = float(valid.mean())
    print("%s: %.0f %% covered, %d distinct triangles visible" % (name, 100 * cover, np.unique(ids[valid]).size))
    assert 0.2 < cover <= 1.0
    assert np.unique(ids[valid]).size >= 10
    # slivers: a visible triangle whose |det| is below a tenth of the six products it is made of (the permanent of |M|)
    c = sc.clip.astype(np.float64)[:, sc.tris]                                   # [B,T,corner,4]
    M = np.abs(np.stack([c[..., 0], c[..., 1], c[..., 3]], 2))                   # [B,T,k,j]
    det = np.linalg.det(np.stack([c[..., 0], c[..., 1], c[..., 3]], 2))
    size = sum(M[:, :, 0, p] * M[:, :, 1, q] * M[:, :, 2, s] for p, q, s in
               ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))) + 1e-300
    seen = np.zeros((sc.B, sc.T), bool)
    for b in range(sc.B):
        seen[b, np.unique(ids[b][valid[b]])] = True
    thin = np.abs(det)[seen] / size[seen]
    print("%s: thinnest visible triangle |det| / products %.1e" % (name, thin.min()))
    assert thin.min() < 0.1


def test_sphere_has_sub_pixel_triangles():
    sc, ids, bary, _ = scene_truth("sphere")
    assert (sc.B, sc.W, sc.H) == (2, 128, 96)
    valid = rs.valid_pixels(ids, bary, sc.T)
    assert 0.3 < float(valid.mean()) < 0.95
    counts = np.bincount(ids[0][valid[0]], minlength=sc.T)
    assert (counts == 1).sum() >= 10, "one-pixel triangles"


@pytest.mark.parametrize("name,size", [("tiny_1x1", (1, 1)), ("tiny_7x3", (7, 3)), ("tiny_64x4", (64, 4))])
def test_tiny_images_are_smaller_than_a_strip(name, size):
    sc, ids, bary, _ = scene_truth(name)
    assert (sc.W, sc.H) == size and sc.W <= 64 and sc.H <= 4
    assert rs.valid_pixels(ids, bary, sc.T).any()
    assert rs.scene("tiny_1x1").clip.tobytes() == sc.clip.tobytes()          # one soup at three sizes


def test_auto16_keeps_sixteen_rows_under_the_automatic_rule():
    sc = rs.scene("auto16")
    assert (sc.B, sc.W, sc.H) == (128, 8, 1024)
    # lanes_rows_per_wave (run_accum.h): halve while B * ceil(W / 64) * ceil(H / rows) < 8192
    rows = 16
    while rows > 4 and sc.B * -(-sc.W // 64) * -(-sc.H // rows) < 8192:
        rows //= 2
    assert rows == 16
    for name in rs.SCENES:
        if name != "auto16":
            s, rows = rs.scene(name), 16
            while rows > 4 and s.B * -(-s.W // 64) * -(-s.H // rows) < 8192:
                rows //= 2
            assert rows == 4, name


@pytest.mark.parametrize("name", rs.SCENES)
def test_reference_alone_sits_inside_the_model(name):
    sc, ids, bary, t = scene_truth(name)
    rel = rs.relative_to_largest(t.o, t)
    print("%-13s r %.3f  K_scene %.1f  max|d| %.3e  oracle max|o - d| / max|d| per image: %s  non-finite truth entries %d" % (
        name, t.r, t.K, float(np.abs(t.d[t.finite]).max()), " ".join("%.1e" % x for x in rel[:4]), int((~t.finite).sum())))
    assert t.finite.mean() > 0.9                       # the truth exists (a degenerate triangle that owns a pixel has none)
    assert float(np.abs(t.d[t.finite]).max()) > 0.0
    assert t.r <= 1.0, "the reference is %.2f times the model's unit away from the truth" % t.r
    assert t.K == 4.0
    assert np.all(t.d[..., 2][t.finite[..., 2]] == 0.0)   # z never receives gradient


@pytest.mark.parametrize("name", rs.DET_SCENES)
def test_deterministic_scenes_stay_inside_the_fixed_point_range(name):
    sc, ids, bary, t = scene_truth(name)
    print("%-13s max per-pixel partial / max|dbary| = 2^%.1f" % (name, np.log2(max(t.max_partial, 1e-300) / t.gmax)))
    assert t.det_headroom_ok(), (t.max_partial, t.gmax)
    assert t.finite.all()
    # the quantisation term: one fixed-point conversion per run and sum, half a quantum each at most
    _, feeding = rs.run_regimes(ids, bary, sc.tris, sc.V)
    quant = feeding.max() * rs.DET_QUANTUM * t.gmax
    print("%-13s most runs feeding one vertex %d: quantisation <= %.2e (floor %.0e)" % (name, feeding.max(), quant, rs.FLOOR))
    assert quant < rs.FLOOR


def test_edited_gbuffer_poisons_every_guarded_case():
    sc = rs.scene("soup_70x37")
    ids, bary = gbuffer("soup_70x37")
    e = rs.edit_gbuffer(sc, ids, bary)
    tris, ids_p, bary_p, ids_c, bary_c, poisoned = (e[k] for k in ("tris", "ids_p", "bary_p", "ids_c", "bary_c", "poisoned"))
    T = tris.shape[0]
    assert T == sc.T + 1 and tris[-1, 0] == sc.V
    for bad in (T, -1, 2 ** 30, sc.T):
        assert (ids_p == bad).sum() == 40 and poisoned[ids_p == bad].all()
    # the appended triangle's pixels sit where no run of the deterministic kernel is open (edit_gbuffer's docstring) ...
    assert set(np.nonzero(ids_p == sc.T)[1]) <= {0, 32}
    # ... and 40 more of them anywhere in the scattered variant
    extra = (e["ids_s"] == sc.T) & (ids_p != sc.T)
    assert extra.sum() == 40 and (e["ids_sc"][extra] == 0).all() and (e["bary_sc"][extra] == 0).all()
    assert np.array_equal(e["ids_s"][~extra], ids_p[~extra]) and np.array_equal(e["ids_sc"][~extra], ids_p[~extra])
    assert len(set(np.nonzero(extra)[1]) - {0, 32}) > 10
    s = (bary_p[..., 0] + bary_p[..., 1]) + bary_p[..., 2]
    below, above = (ids_p == 0) & (s < rs.CUTOFF) & (s > 0.89), (ids_p == 0) & (s >= rs.CUTOFF) & (s < 0.91)
    assert below.sum() == 40 and above.sum() == 40 and poisoned[below].all() and not poisoned[above].any()
    # the clean buffer: poisoned pixels are background, everything else untouched; no pixel names the appended triangle
    assert (ids_c[poisoned] == 0).all() and (bary_c[poisoned] == 0).all()
    assert np.array_equal(ids_c[~poisoned], ids_p[~poisoned]) and np.array_equal(bary_c[~poisoned], bary_p[~poisoned])
    valid_p, valid_c = rs.valid_pixels(ids_p, bary_p, T), rs.valid_pixels(ids_c, bary_c, T)
    assert np.array_equal(valid_p & ~(ids_p == sc.T), valid_c) and (ids_c < sc.T).all() and (ids_c >= 0).all()
    t = rs.truth(sc, ids_c, bary_c, key="edited")
    print("edited: r %.3f K_scene %.1f" % (t.r, t.K))
    assert t.r <= 1.0 and t.K == 4.0 and t.det_headroom_ok() and t.finite.all()
    # the pixels of triangle 0 with a sum just above 0.9 do contribute: the truth differs from the one without them
    ids_z, bary_z = ids_c.copy(), bary_c.copy()
    bary_z[above] = 0.0
    assert np.abs(rs.truth(sc, ids_z, bary_z, key="edited, without the pixels above 0.9").d - t.d).max() > 0
