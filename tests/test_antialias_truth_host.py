"""The antialiasing truth on the host: the scenes of tests/antialias_scenes.py reach the regimes they are named for, the
two spellings of rule 8 (tests/antialias_reference.py) agree, and the float32 restatement stays inside the noise model
that bounds the kernels in tests/test_antialias_truth_gpu.py (no GPU needed; the G-buffer is oracle.forward's).

THE BOUND.  Elementwise |kernel - truth| <= K 2^-24 noise + 1e-7 max|truth|, noise from the truth's own terms
(pair_gradients / blend / blend_backward).  r32 is the largest |float32 restatement - truth| / (2^-24 noise); K is
4 r32 rounded up to a power of two, the factor 4 for the kernel's different, equally long order of summation (the
butterfly's six steps and the atomic commits).  Measured here, never on a kernel:

    scene            r32 out   dimage   dclip        scene            r32 out   dimage   dclip
    ragged_65x47     1.35      1.69     0.17         centre           0.72      0.86     0.28
    ragged_63x5      1.16      1.09     1.16         coplanar         1.04      1.25     0.21
    ragged_7x3       0.43      0.53     0.50         rolled_1         0.85      1.49     0.12
    ragged_130x6     0.85      1.25     0.53         rolled_2         0.97      1.10     0.14
    ragged_1x9       1.08      0.91     1.15         poisoned         0.92      1.31     0.11
    ragged_9x1       0.41      0.24     0.06         scaled_1         1.52      2.14     0.70
    seams_sphere     0.89      1.77     0.31         scaled_down      1.52      2.14     0.70
    seams_soup       1.57      1.91     1.02         scaled_up        1.52      2.14     0.70
    long_edge        1.18      1.43     0.42         spike            0.43      0.91     0.59
    (ragged_65x47: the worst of C = 1, 2, 3, 4, 5, 7; ragged_1x1, midpoint, no_triangles, no_images blend nothing;
    seams_soup with the image times 1e3 / 1e-3: 2.05 / 1.93)

    r32 = 2.14 (scaled_1, dimage)  ->  4 r32 = 8.6  ->  K = 16 (antialias_scenes.K)

THE CLAMPED CASE (rules 5 and 8).  Where t was clamped the crossing point is the end of the segment the clamp chose and
dt/dv is the literal formula's there; the derivative of the unclamped quotient is another number (rolled_1: 66 of 110
pairs with t == 0; rolled_2: 71 with t == 0 and 3 with t == 1 of 100; with these inputs the two spellings differ by
2.5 and 3.2 times the largest gradient).  Where 0 < t < 1 the literal formula at the float64 quotient is the quotient's
derivative to 1e-12; the truth forms P_c from the decided float32 t, as rule 8 and the kernel do.  antialias() and
pair_gradients() are asserted equal on every scene.
"""
import numpy as np
import pytest
import torch

import antialias_reference as ref
import antialias_scenes as S

K = S.K


def _truth(name, C=None, image_scale=1.0):
    sc, g, pairs, mask = S.host(name)
    image, dout = sc.inputs(C, image_scale)
    return sc, pairs, image, dout, S.Truth(sc, pairs, image, dout)


# ---- the scenes reach their regimes -------------------------------------------------------------------------------------
def test_ragged_sizes_fit_no_tile_and_still_blend():
    for (W, H), name in zip(S.RAGGED_SIZES, S.RAGGED):
        sc, _, pairs, mask = S.host(name)
        assert (sc.W, sc.H, sc.B) == (W, H, 2)
        assert W % S.TILE_W != 0 and (H % S.TILE_H != 0 or W % S.TILE_W != 0)
        r = S.regimes(sc, pairs, mask)
        assert r["pairs"] > 0 or (W, H) == (1, 1), name
    assert any(H % S.TILE_H for _, H in S.RAGGED_SIZES)             # whole wavefronts out of range
    assert S.regimes(*_three("ragged_1x1"))["candidates"] == 0      # no pair at all
    assert S.regimes(*_three("ragged_130x6"))["seam_x"] >= 1 and S.regimes(*_three("ragged_63x5"))["seam_y"] >= 1
    assert S.regimes(*_three("ragged_65x47"))["seam_y"] >= 1


def _three(name):
    sc, _, pairs, mask = S.host(name)
    return sc, pairs, mask


def test_seams_scenes_blend_across_both_kinds_of_seam_with_many_vertices_per_wavefront():
    soup = S.regimes(*_three("seams_soup"))
    assert soup["seam_x"] >= 1 and soup["seam_y"] >= 1
    assert soup["wave_most_vertices"] >= 16
    assert soup["mask15"] >= 1 and soup["lane_repeat"] >= 1
    sphere = S.regimes(*_three("seams_sphere"))
    assert sphere["pairs"] >= 20 and sphere["candidates"] > 4 * sphere["pairs"]    # mostly interior edges: rule 6 rejects


def test_long_edge_puts_whole_wavefronts_on_two_vertices():
    r = S.regimes(*_three("long_edge"))
    assert r["wave_two_vertices"] >= 60, r
    sc, _, pairs, _ = S.host("long_edge")
    assert pairs["horizontal"].any() and (~pairs["horizontal"]).any()


def test_spike_is_one_pixel_modified_by_all_four_pairs():
    sc, g, pairs, mask = S.host("spike")
    r = S.regimes(sc, pairs, mask)
    assert (r["pairs"], r["mask15"], r["candidates"]) == (4, 1, 4)
    assert r["lane_repeat"] == 3                                     # each of the three vertices in several slots
    assert (g[4] == -1).all()
    assert pairs["mod_f"].all() and len({(int(y), int(x)) for y, x in zip(pairs["my"], pairs["mx"])}) == 1


def test_midpoint_blends_nothing_and_centre_blends_everything_at_t_zero():
    def outline_of(g, c):                                           # the candidates with exactly one covered pixel
        cov = (g[0] != 0) | (g[1].sum(-1) >= 0.9)
        return cov[c["b"], c["ay"], c["ax"]] != cov[c["b"], c["by"], c["bx"]]
    sc, g, pairs, mask = S.host("midpoint")
    c = pairs["candidates"]
    outline = outline_of(g, c)
    assert int(outline.sum()) == 8 and c["half"][outline].all() and not c["blended"].any()
    assert not mask.any()
    sc, g, pairs, mask = S.host("centre")
    c = pairs["candidates"]
    outline = outline_of(g, c)
    assert int(outline.sum()) == 8 and c["blended"][outline].all() and int(c["blended"].sum()) == 8
    assert (pairs["t"] == 0).all() and pairs["mod_f"].all()
    assert (ref._weights(pairs, np.float32) == 0.5).all()


def test_coplanar_pairs_are_decided_by_the_larger_id():
    sc, g, pairs, mask = S.host("coplanar")
    r = S.regimes(sc, pairs, mask)
    assert r["equal_z_blended"] >= 5
    ids, z = g[0], g[2]
    b = pairs["b"]
    idf, idg = ids[b, pairs["fy"], pairs["fx"]], ids[b, pairs["gy"], pairs["gx"]]
    both = (z[b, pairs["fy"], pairs["fx"]] == z[b, pairs["gy"], pairs["gx"]]) & (idf != idg)
    cov_g = (idg != 0) | (g[1][b, pairs["gy"], pairs["gx"]].sum(-1) >= 0.9)
    tie = both & cov_g                                               # two covered pixels at one depth
    assert int(tie.sum()) >= 5 and (idf[tie] > idg[tie]).all()


def test_rolled_gbuffers_clamp_t_at_both_ends():
    r1, r2 = S.regimes(*_three("rolled_1")), S.regimes(*_three("rolled_2"))
    assert r1["t0"] >= 20 and r2["t0"] >= 20 and r2["t1"] >= 1, (r1, r2)
    own = S.regimes(*_three("ragged_65x47"))
    assert own["t0"] == own["t1"] == 0                               # the rasterizer's own G-buffer never clamps


def test_poisoned_pairs_are_candidates_and_never_blend():
    import oracle
    sc, g, pairs, mask = S.host("poisoned")
    ids, tris, opp = g[0], g[3], g[4]
    clean = oracle.forward(sc.clip, sc.tris, sc.W, sc.H)[0]
    bad_px = ids != clean
    assert sorted(set(ids[bad_px].tolist())) == sorted([S.INT32_MIN, -1, sc.T, sc.T + 7])
    assert 10 <= int(bad_px.sum()) <= 12
    cov = (clean != 0) | (g[1].sum(-1) >= 0.9)
    assert int((bad_px & cov).sum()) >= 3 and int((bad_px & ~cov).sum()) >= 6
    c = pairs["candidates"]
    touches = bad_px[c["b"], c["ay"], c["ax"]] | bad_px[c["b"], c["by"], c["bx"]]
    assert int(touches.sum()) >= 24                                 # poisoned pixels next to covered and to uncovered ones
    front_is_bad = touches & ~c["blended"]
    assert int(front_is_bad.sum()) >= 16                            # present in the candidate set, absent from the blended
    b = pairs["b"]
    F = ids[b, pairs["fy"], pairs["fx"]]
    assert ((F >= 0) & (F < sc.T)).all()                            # no blended pair has a poisoned front pixel ...
    assert bad_px[b, pairs["gy"], pairs["gx"]].any()                # ... but some have one as g
    bad_tri = np.nonzero((tris >= sc.V).any(1))[0]
    assert len(bad_tri) == 1 and (clean == bad_tri[0]).sum() > 50 and not (F == bad_tri[0]).any()
    bad_opp = np.nonzero((opp >= sc.V).any(1))[0]
    assert len(bad_opp) == 1 and (clean == bad_opp[0]).sum() > 50
    # the triangle with the poisoned topology still blends through its boundary-free edges only: its blended pairs'
    # exit edges are not the poisoned ones
    for va, vb in zip(pairs["va"][F == bad_opp[0]], pairs["vb"][F == bad_opp[0]]):
        k = [k for k in range(3) if {int(tris[bad_opp[0], (k + 1) % 3]), int(tris[bad_opp[0], (k + 2) % 3])} == {int(va), int(vb)}]
        assert len(k) == 1 and opp[bad_opp[0], k[0]] < sc.V
    fewer = len(S.host("ragged_65x47")[2]["b"])
    assert len(b) < fewer                                            # the poison took pairs away
    for name in ("poisoned", "rolled_1", "rolled_2"):
        t = _truth(name)[4]
        assert all(np.isfinite(a).all() for a in (t.out, t.dimage, t.dclip, t.n_dclip))


def test_scaling_clip_by_a_power_of_two_moves_no_decision():
    base = S.host("scaled_1")
    for name in ("scaled_down", "scaled_up"):
        sc, g, pairs, mask = S.host(name)
        assert all(np.array_equal(a, b) for a, b in zip(g[:3], base[1][:3]))          # the same G-buffer, bit for bit
        assert np.array_equal(mask, base[3]) and np.array_equal(pairs["t"], base[2]["t"])
        image, dout = sc.inputs()
        assert np.array_equal(image, base[0].inputs()[0])
        a = ref.pair_gradients(image, dout, sc.clip, pairs, np.float32)[0]
        b = ref.pair_gradients(image, dout, base[0].clip, base[2], np.float32)[0]
        assert np.array_equal(a * sc.scale, b)                        # the float32 restatement: a power of two moves no rounding


def test_empty_scenes_have_no_candidates():
    for name in ("no_triangles", "no_images"):
        sc, g, pairs, mask = S.host(name)
        assert len(pairs["candidates"]["b"]) == 0 and not mask.any()
        t = _truth(name)[4]
        assert t.dclip.shape == sc.clip.shape and not t.dclip.any()


# ---- the two spellings of rule 8 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.SCENES)
def test_literal_formula_equals_the_autograd_spelling(name):
    sc, pairs, image, dout, t = _truth(name)
    if len(pairs["b"]) == 0:
        return
    sa, sb, t64 = ref.autograd_slopes(sc.clip, pairs)
    inside = (pairs["t"] > 0) & (pairs["t"] < 1)
    p = ref.pair_terms(image, dout, sc.clip, pairs, t=np.where(inside, t64, pairs["t"]))
    assert float(np.abs(t64 - pairs["t"])[inside].max(initial=0.0)) < 1e-4     # the decided t is that quotient, in float32
    for lit, auto in ((p["slope_a"], sa), (p["slope_b"], sb)):
        size = np.abs(lit).max(1, keepdims=True)                    # the pair's magnitude
        assert (np.abs(lit - auto)[inside] <= 1e-12 * size[inside]).all()
    # ... and antialias(), whose slope on the clamped pairs is the literal one, gives pair_gradients' sums
    img64 = torch.tensor(image, dtype=torch.float64, requires_grad=True)
    clip64 = torch.tensor(sc.clip, dtype=torch.float64, requires_grad=True)
    out = ref.antialias(img64, clip64, pairs)
    (out * torch.tensor(dout, dtype=torch.float64)).sum().backward()
    scale = max(float(np.abs(t.dclip).max()), 1e-300)
    assert float(np.abs(clip64.grad.numpy() - t.dclip).max()) <= 1e-12 * scale
    assert float(np.abs(out.detach().numpy() - t.out).max()) <= 1e-14 * max(float(np.abs(t.out).max()), 1.0)
    assert float(np.abs(img64.grad.numpy() - t.dimage).max()) <= 1e-14 * max(float(np.abs(t.dimage).max()), 1.0)
    assert not t.dclip[..., 2].any()


def test_unclamped_derivative_is_another_number_where_t_is_clamped():
    """What gap 3 of the issue measured: on the rolled G-buffers the derivative of the unclamped quotient is far from
    rule 8's (15 % and 160 % of the largest gradient there); the suite now pins rule 8's."""
    for name, least in (("rolled_1", 0.05), ("rolled_2", 0.5)):
        sc, pairs, image, dout, t = _truth(name)
        p = ref.pair_terms(image, dout, sc.clip, pairs)
        sa, sb, _ = ref.autograd_slopes(sc.clip, pairs)
        other = np.zeros_like(t.dclip)
        for v, s in ((pairs["va"], sa), (pairs["vb"], sb)):
            for i, col in enumerate((0, 1, 3)):
                np.add.at(other[..., col], (pairs["b"], v), p["dldt"] * s[:, i])
        rel = float(np.abs(other - t.dclip).max() / np.abs(t.dclip).max())
        print("AAT | %-9s | unclamped-quotient spelling differs by %.2f of max|dclip|" % (name, rel))
        assert rel > least


# ---- the reference alone stays inside the model ------------------------------------------------------------------------
def test_float32_restatement_sets_K():
    worst, where = 0.0, None
    for name in S.SCENES:
        for C in (S.CHANNELS if name == S.FULL_SWEEP else (None,)):
            t = _truth(name, C)[4]
            print("AAT | %-13s C %s | r32 out %.2f dimage %.2f dclip %.2f" % (
                name, C or S.scene(name).C, t.r32["out"], t.r32["dimage"], t.r32["dclip"]))
            for k, v in t.r32.items():
                if v > worst:
                    worst, where = v, (name, C, k)
    print("AAT | r32 = %.3f at %s -> K = %g" % (worst, where, K))
    assert 4.0 * worst <= K, (worst, where)
    assert K < 8.0 * worst, (worst, K)                              # ... and K is the next power of two, no looser
    # the float32 restatement itself is inside the bound with the factor 4 to spare
    for name in S.SCENES:
        t = _truth(name)[4]
        sc, pairs, image, dout = _truth(name)[:4]
        f32 = ref.pair_gradients(image, dout, sc.clip, pairs, np.float32)[0]
        assert ref.excess(f32, t.dclip, t.n_dclip, K / 4.0) <= 1.0


def test_noise_scale_carries_the_conditioning_of_D():
    """Without cond_d the model is off by tens of units on small images (the issue: a 7 x 3 cube at 40)."""
    sc, pairs, image, dout, t = _truth("ragged_7x3")
    p = ref.pair_terms(image, dout, sc.clip, pairs)
    assert float(p["cond_d"].max()) > 1.0 and np.isfinite(p["cond_d"]).all()
    assert (p["dldt_abs"] >= np.abs(p["dldt"])).all()


def test_image_scale_does_not_move_the_ratio():
    for scale in (1e3, 1e-3):
        t = _truth("seams_soup", image_scale=scale)[4]
        assert max(t.r32.values()) <= K / 4.0
        assert float(np.abs(t.out).max()) > 0.5 * scale
