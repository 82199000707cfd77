"""Which pixel-pass kernel the shading backward launches for which call (DESIGN.md 4.4's decision table).

`expected()` and `expected_specular()` restate the table in Python, independently of the C++ that implements it
(plan_shade_backward / plan_spec_backward); the sweeps call the library over the whole grid of caller
combinations and compare mr_debug_last_accumulate_kernel's functor spelling, case by case."""
import collections
import itertools

import pytest
import torch

from pytorch_mesh_renderer_amd.common import shapes, synthetic

pytestmark = pytest.mark.gpu

B, W, H = 2, 32, 24
REJECTED = "rejected"

Case = collections.namedtuple("Case", "L signs light_grads normals diffuse clip normalised records prepared "
                                      "adjacency transforms deterministic kernel")


def _spell(name, args, defaults=()):
    """The functor as the compiler spells it: trailing template arguments that equal their defaults are left out."""
    args = list(args)
    for default in reversed(defaults):
        if args[-1] != default:
            break
        args.pop()
    return "%s<%s>" % (name, ", ".join(str(a).lower() if isinstance(a, bool) else str(a) for a in args))


def expected(c):
    """Case -> functor spelling of the pixel pass, or REJECTED (MR_EINVAL)."""
    groups = int(c.normals) | 2 | int(c.diffuse) << 2
    nl = c.L if c.L <= 4 else 0
    if c.deterministic and not c.adjacency:
        return REJECTED
    lights_fit = not c.light_grads or c.L <= 2       # the lane kernels carry the light gradients of one or two lights
    fold = (not c.clip and c.transforms and not c.deterministic and c.normalised and c.kernel != 1 and groups != 6 and
            ((lights_fit and c.records) if c.light_grads else (groups == 2 or c.records or c.prepared)))
    fold_diff = fold and (c.records or c.prepared) and groups == 2 and not c.light_grads
    diff = (not fold_diff and c.records and c.adjacency and c.normalised and not c.deterministic and c.kernel != 1 and
            groups != 6 and lights_fit)
    if fold and not fold_diff and not diff:
        return REJECTED          # folding wanted, but the difference-basis kernels need records the caller did not give
    if c.light_grads and c.L > 4:
        return REJECTED
    if not (c.normals and c.diffuse) and not c.adjacency:
        return REJECTED
    lanes = not c.deterministic and groups != 6 and c.kernel != 1 and lights_fit
    if diff and lanes:
        return _spell("ShadeDiffLaneFn", (nl, c.signs, groups, fold, c.light_grads), (False,))
    if lanes and fold_diff:
        return _spell("ShadeFoldLaneFn", (nl, c.signs))
    if lanes and c.light_grads:
        return _spell("ShadeLaneFn", (nl, c.signs, True, groups, False, False), (False, False))
    if lanes:
        return _spell("ShadeLaneFn", (nl, c.signs, False, groups, c.normalised, False), (False, False))
    return _spell("ShadeGradFn", (nl, c.signs, c.light_grads))


def _scene(device, n_lights):
    vertices, triangles, normals = shapes.cube(2.0)
    triangles = torch.flip(triangles, [1]).contiguous()   # CCW -> CW, as the examples do
    gen = torch.Generator().manual_seed(11)
    eyes = torch.tensor([[2.0, 3.0, 6.0], [-3.0, 2.0, 5.0]])
    s = {"vertices": vertices.unsqueeze(0).repeat(B, 1, 1).contiguous(), "triangles": triangles,
         "normals": normals.unsqueeze(0).repeat(B, 1, 1).contiguous(),
         "diffuse": torch.rand(B, 8, 3, generator=gen) * 0.8 + 0.2,
         "light_positions": torch.rand(B, n_lights, 3, generator=gen) * 6 - 3 + torch.tensor([0.0, 0.0, 6.0]),
         "light_intensities": torch.rand(B, n_lights, 3, generator=gen) * 0.5 + 0.2,
         "ambient": torch.rand(B, 3, generator=gen) * 0.3,
         "transforms": synthetic.clip_transforms(eyes, W, H), "eyes": eyes,
         "dense": torch.randn(B, H, W, 4, generator=gen) / (H * W)}
    return {k: v.to(device) for k, v in s.items()}


def test_shade_backward_launches_the_kernel_the_decision_table_names(device):
    """Unit cube (8 vertices, 12 triangles), two images of 32 x 24: every family launches at that size, the lane
    kernels halve their strips down to 4 rows, the rows kernel has one partial strip.  Per case: the functor that
    ran is expected()'s; a rejected case raises "invalid argument"; an accepted one returns finite gradients and
    None exactly for what was not wanted.  Combinations _shade_backward_call itself refuses (ValueError) are skipped."""
    from pytorch_mesh_renderer_amd import _native
    bools = (False, True)
    failures, finite, n_cases, n_rejected = [], [], 0, 0
    try:
        for L in (1, 2, 3, 4, 5):
            s = _scene(device, L)
            fwd = lambda **kw: _native.render_forward(
                s["vertices"], s["transforms"], s["normals"], s["diffuse"], s["triangles"], s["light_positions"],
                s["light_intensities"], s["ambient"], W, H, want_z=False, **kw)
            clip, ids, bary, _, rgba, records, pristine = fwd(prepare_backward=True)
            _, signs = _native.l1_loss_forward(rgba, torch.zeros_like(rgba))
            up = torch.full((1,), 0.7, device=device)
            adjacency = _native.vertex_adjacency(s["triangles"], 8)
            tail = (ids, bary, clip, s["normals"], s["vertices"], s["diffuse"], s["triangles"], s["light_positions"],
                    s["light_intensities"], s["ambient"])
            for (sg, lg, n, d, cl, nrm, rec, prep, (adj, xf), det, k) in itertools.product(
                    bools, bools if L <= 4 else (False,), bools, bools, bools, bools, bools, bools,
                    ((False, False), (True, False), (True, True)), bools, (0, 1)):
                c = Case(L, sg, lg, n, d, cl, nrm, rec, prep, adj, xf, det, k)
                if (not cl and not xf) or (not (n and d) and not adj):
                    continue   # _shade_backward_call raises ValueError
                prepared = None
                if prep:   # a block serves one backward: a fresh copy of the forward's per call
                    prepared = _native._aligned_bytes(pristine.numel(), device)
                    prepared.copy_(pristine)
                _native.set_deterministic(det)
                _native.debug_set_shade_backward_kernel(k)
                kw = dict(corner_records=records if rec else None, adjacency=adjacency if adj else None,
                          l1_signs=signs if sg else None, transforms=s["transforms"] if xf else None,
                          want_light_grads=lg, want_normal_grads=n, want_diffuse_grads=d, normalised_gbuffer=nrm,
                          want_clip_grads=cl, prepared=prepared)
                want = expected(c)
                n_cases += 1
                try:
                    out = _native._shade_backward_call(up if sg else s["dense"], *tail, **kw)
                except RuntimeError as e:
                    n_rejected += 1
                    if want != REJECTED or "invalid argument" not in str(e):
                        failures.append("%s: expected %s, raised %s" % (c, want, e))
                    continue
                ran = _native.debug_last_accumulate_kernel()
                if ran != want:
                    failures.append("%s: expected %s, ran %s" % (c, want, ran))
                    continue
                none_pattern = tuple(o is None for o in out)
                if none_pattern != (not cl, not n, False, not d, not lg, not lg, not lg):
                    failures.append("%s: outputs left out %s" % (c, none_pattern))
                finite.append((c, torch.cat([o.reshape(-1) for o in out if o is not None]).isfinite().all()))
    finally:
        _native.set_deterministic(False)
        _native.debug_set_shade_backward_kernel(0)
    ok = torch.stack([f for _, f in finite]).cpu().tolist()
    failures += ["%s: a gradient is not finite" % (c,) for (c, _), good in zip(finite, ok) if not good]
    print("shade backward dispatch: %d cases, %d rejected" % (n_cases, n_rejected))
    assert n_cases > 5000 and n_rejected > 0
    assert not failures, "%d of %d cases:\n%s" % (len(failures), n_cases, "\n".join(failures[:20]))


def expected_specular(L, per_vertex, grads_wanted, normalised, transforms, signs, deterministic):
    """-> functor spelling of mr_shade_specular_backward's pixel pass (the adjacency is always given)."""
    from pytorch_mesh_renderer_amd import _native
    lanes = not deterministic and normalised and (grads_wanted & ~(_native.GRAD_POSITIONS | _native.GRAD_CLIP)) == 0
    fold = lanes and transforms and not grads_wanted & _native.GRAD_CLIP
    if fold and L <= 2:   # one pass; the only pixel kernel that reads sign codes (the others get them made dense first)
        return _spell("SpecCoupledLaneFn", (L, per_vertex, signs), (False,))
    if lanes:
        return _spell("SpecFoldLaneFn", (L, per_vertex, fold))
    return _spell("SpecGradFn", (L, per_vertex, False), (False,))


def test_shade_specular_backward_launches_the_kernel_the_decision_table_names(device):
    from pytorch_mesh_renderer_amd import _native
    bools = (False, True)
    sets = ((_native.GRAD_ALL, False, False),                                     # the three calls of backward_fuzz
            (_native.GRAD_POSITIONS | _native.GRAD_CLIP, True, False),
            (_native.GRAD_POSITIONS, True, True))
    failures, finite, n_cases = [], [], 0
    gen = torch.Generator().manual_seed(12)
    specular = (torch.rand(B, 8, 3, generator=gen) * 0.5).to(device)
    try:
        for L in (1, 2, 3, 4):
            s = _scene(device, L)
            clip, ids, bary, _, _, _ = _native.render_forward(
                s["vertices"], s["transforms"], s["normals"], s["diffuse"], s["triangles"], s["light_positions"],
                s["light_intensities"], s["ambient"], W, H, want_z=False)
            adjacency = _native.vertex_adjacency(s["triangles"], 8)
            up = torch.full((1,), 0.7, device=device)
            for pv in bools:
                shininess = (torch.rand(B, 8, generator=gen) * 20 + 5 if pv else torch.tensor([10.0, 25.0])).to(device)
                args = (ids, bary, s["normals"], s["vertices"], s["diffuse"], specular, s["triangles"], s["light_positions"],
                        s["light_intensities"], s["ambient"], s["eyes"], shininess)
                rgba, norms2 = _native.shade_specular_forward(*args)
                _, signs = _native.l1_loss_forward(rgba, torch.zeros_like(rgba))
                for (gw, nrm, xf), sg, det in itertools.product(sets, bools, bools):
                    _native.set_deterministic(det)
                    out = _native.shade_specular_backward(
                        up if sg else s["dense"], ids, bary, clip, *args[2:], norms2, adjacency=adjacency,
                        transforms=s["transforms"] if xf else None, normalised_gbuffer=nrm, grads_wanted=gw,
                        l1_signs=signs if sg else None)
                    n_cases += 1
                    what = "L=%d per-vertex %s grads %d signs %s deterministic %s" % (L, pv, gw, sg, det)
                    want, ran = expected_specular(L, pv, gw, nrm, xf, sg, det), _native.debug_last_accumulate_kernel()
                    if ran != want:
                        failures.append("%s: expected %s, ran %s" % (what, want, ran))
                    # (what was not asked for comes back unspecified)
                    read = out if gw == _native.GRAD_ALL else (out[0], out[2]) if gw & _native.GRAD_CLIP else (out[2],)
                    finite.append((what, torch.cat([o.reshape(-1) for o in read]).isfinite().all()))
    finally:
        _native.set_deterministic(False)
    ok = torch.stack([f for _, f in finite]).cpu().tolist()
    failures += ["%s: a gradient is not finite" % what for (what, _), good in zip(finite, ok) if not good]
    print("specular backward dispatch: %d cases" % n_cases)
    assert n_cases == 96
    assert not failures, "%d of %d cases:\n%s" % (len(failures), n_cases, "\n".join(failures[:20]))
