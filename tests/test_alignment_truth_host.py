"""What tests/test_alignment_truth_gpu.py leans on, and the torch spelling in the same regimes, without a GPU.

The condition: every case of tests/alignment_regimes.py states whether its R is unique, per reflection flag, and the
truth's g = sigma_2 + e sigma_3 has to agree, so that no case slides from the entry-by-entry comparison to the
residual comparison unseen; the slabs' third singular value crosses the kernels' rank tolerance of 1e-13 between
2^-21 and 2^-22.  The torch spelling (float64) is held to the numpy restatement at 1e-12 where R is unique and through
its residual elsewhere, and a row that is not counted -- weight 0, at coordinates of 1e4, 1e6 and 3e38 -- changes
nothing, wherever it sits."""
import itertools

import numpy as np
import pytest
import torch

import alignment_regimes as regimes
from pytorch_mesh_renderer_amd import mesh_renderer

points = mesh_renderer.points
TOL = 1e-12


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def test_every_case_is_in_the_regime_it_states():
    ratios = {}
    for name, x, y, w, expects, family in regimes.regime_cases():
        for reflect in (False, True):
            want, _, sigma, e, g, unique = regimes.truth(x, y, w, True, reflect)
            assert unique == expects[reflect], (name, reflect, g, sigma)
            det = np.linalg.det(want.R)
            assert abs(det - 1) <= 1e-12 or (reflect and abs(det + 1) <= 1e-12), (name, det)
        ratios[name] = sigma[2] / sigma[0]
    base = regimes.truth(*regimes.regime_cases()[0][1:4], True, False)
    print("base cloud: sigma_3 / sigma_1 = %.3g, g / sigma_1 = %.3g" % (base[2][2] / base[2][0], base[4]))
    slabs = [ratios["slab 2^-%d" % t] for t in regimes.SLAB_EXPONENTS]
    print("slabs: sigma_3 / sigma_1 =", " ".join("%.2g" % v for v in slabs))
    assert all(a > b for a, b in zip(slabs, slabs[1:]))
    assert slabs[0] > 1e-6 > slabs[1] and slabs[5] > 1e-13 > slabs[6]          # t = 8 | 12 and t = 21 | 22
    assert ratios["planar"] <= 1e-15 and ratios["planar mirrored in the plane"] <= 1e-15
    assert abs(ratios["cube"] - 1) <= 1e-6 and abs(ratios["cube (1,1,0.5)"] - 0.25) <= 1e-6


def test_the_planted_transforms_are_found_by_the_truth():
    """The truth itself: a signed permutation comes back exactly (y is exact), a mirror comes back as the mirror with
    reflection allowed, and as a proper rotation with s = (sigma_1 + sigma_2 - sigma_3) / var x without."""
    for (name, P), case in zip(regimes.signed_permutations(), regimes.regime_cases()):
        assert case[0] == name
        want = regimes.truth(case[1], case[2], None, True, True)[0]
        assert np.abs(want.R - P).max() <= 1e-13 and abs(want.s - regimes.SCALE) <= 1e-13
        assert np.abs(want.T - regimes.SHIFT).max() <= 1e-13
    mirror = next(c for c in regimes.regime_cases() if c[0] == "mirror")
    free, _, sigma, _, _, _ = regimes.truth(mirror[1], mirror[2], None, True, True)
    assert np.linalg.det(free.R) < 0 and abs(free.s - regimes.SCALE) <= 1e-6
    proper = regimes.truth(mirror[1], mirror[2], None, True, False)[0]
    var_x = regimes.variance(mirror[1], None)
    assert abs(np.linalg.det(proper.R) - 1) <= 1e-12 and abs(proper.s - (sigma[0] + sigma[1] - sigma[2]) / var_x) <= 1e-12


@pytest.mark.parametrize("scale,reflect", list(itertools.product((False, True), repeat=2)))
def test_torch_spelling_in_every_regime(scale, reflect):
    cases = regimes.regime_cases()
    x, y, w, n = regimes.padded_batch(cases)
    got = points.corresponding_points_alignment(_t(x), _t(y), _t(w), torch.as_tensor(n), estimate_scale=scale,
                                                allow_reflection=reflect)
    for b, (name, cx, cy, cw, expects, _) in enumerate(cases):
        regimes.check(got.R[b].numpy(), got.T[b].numpy(), got.s[b], cx, cy, cw, scale, reflect, expects[reflect],
                      (name, scale, reflect), tol=TOL)
    one = points.corresponding_points_alignment(_t(cases[50][1]), _t(cases[50][2]), estimate_scale=scale,
                                                allow_reflection=reflect)
    regimes.check(one.R.numpy(), one.T.numpy(), one.s, *cases[50][1:4], scale, reflect, cases[50][4][reflect],
                  cases[50][0], tol=TOL)


@pytest.mark.parametrize("placement", range(len(regimes.sentinel_placements())))
def test_a_row_of_weight_zero_influences_nothing_in_the_torch_spelling(placement):
    name, x, y, rows = regimes.sentinel_placements()[placement]
    mirrored = name.startswith("base")
    for reflect in ((False, True) if mirrored else (False,)):
        known = None
        for value in regimes.SENTINELS:
            sx, sy, kept = regimes.with_sentinels(x, y, rows, value)
            known = known or regimes.truth(sx[kept], sy[kept], None, True, reflect)
            got = points.corresponding_points_alignment(_t(sx), _t(sy), _t(kept), estimate_scale=True,
                                                        allow_reflection=reflect)
            print(name, value, "|R - R64| = %.3g" % np.abs(got.R.numpy() - known[0].R).max())
            regimes.check(got.R.numpy(), got.T.numpy(), got.s, sx[kept], sy[kept], None, True, reflect, True,
                          (name, value, reflect), tol=TOL, known=known)


def test_float32_host_tensors_survive_a_far_row_of_weight_zero():
    """The same in float32, where the square of 3e38 overflows: the weight multiplies first, so nothing does."""
    name, x, y, rows = regimes.sentinel_placements()[0]
    sx, sy, kept = regimes.with_sentinels(x, y, rows, 3e38)
    got = points.corresponding_points_alignment(_t(sx, torch.float32), _t(sy, torch.float32), _t(kept, torch.float32),
                                                estimate_scale=True)
    want = regimes.truth(sx[kept], sy[kept], None, True, False)[0]
    assert np.abs(got.R.numpy() - want.R).max() <= 1e-5 and abs(float(got.s) - want.s) <= 1e-5
