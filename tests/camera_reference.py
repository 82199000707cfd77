"""A restatement of the clip-space camera transform, perspective @ look_at, in plain torch on the host (TEST
INFRASTRUCTURE ONLY), the seeded camera families it is evaluated on and the bound the camera kernels
(csrc/mesh_ops.hip: k_camera_transforms, k_camera_transforms_backward) are held to.

The restatement goes through common.camera_utils.look_at / perspective, which follow the dtype of their inputs and
are differentiable: run in float64 on the float32 inputs it is the truth, run in float32 on the CPU it is the
yardstick.  Per family and tensor (the matrix, d eye, d center, d up, and d fov where asked for)

    r = max over cameras b of  max|f32[b] - f64[b]| / max|f64[b]|

and a kernel is allowed, per camera,

    |kernel - f64|[b]  <=  K * r * max|f64[b]|  +  FLOOR * max|f64|          (K = 8, FLOOR = 1e-7: tests/soft_truth.py)

r is taken over the whole family (all SIZE cameras, of which the smaller batches of the tests are prefixes -- the
cameras of a batch are independent, so a prefix of the truth is the truth of the prefix): the float32 error of ONE
camera is a draw from a distribution whose width the family shows, and two float32 evaluations of the same camera are
two draws.

Families (every input is rounded to float32 BEFORE either precision sees it):

    plain            eye ~ 3 N(0,1), center ~ 0.5 N(0,1), up ~ N(0,1) + (0,2,0), fov 10..160 degrees,
                     near 0.01..0.21, far = near + 1..101, all per image
    far_eye          plain with the eye x 300
    long_up          plain with |up| log-uniform over 1e-3 .. 1e3
    near_degenerate  up = gaze + 1e-2 N(0,1)        (gaze: the unit vector from eye to center)
    close            center = eye + 1e-3 N(0,1)
"""
import functools

import torch

from pytorch_mesh_renderer_amd.common import camera_utils
from soft_truth import FLOOR, K

FAMILIES = ("plain", "far_eye", "long_up", "near_degenerate", "close")
SEED = 5
SIZE = 600        # the largest batch of the tests; the smaller ones are its prefixes
ASPECT = 1.5
CUTOFF = camera_utils._DEGENERACY_CUTOFF
INPUTS = ("eye", "center", "up")


def family(name, batch, seed=SEED):
    """-> dict of float32 CPU tensors: eye, center, up [B,3], fov, near, far [B]."""
    g = torch.Generator().manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    eye, center = 3.0 * randn(batch, 3), 0.5 * randn(batch, 3)
    up = randn(batch, 3) + torch.tensor([0.0, 2.0, 0.0], dtype=torch.float64)
    fov = 10.0 + 150.0 * rand(batch)
    near = 0.01 + 0.2 * rand(batch)
    far = near + 1.0 + 100.0 * rand(batch)
    extra, spread = randn(batch, 3), rand(batch)          # drawn for every family: the plain part is common to all
    if name == "far_eye":
        eye = eye * 300.0
    elif name == "long_up":
        up = torch.nn.functional.normalize(up, dim=1) * (10.0 ** (6.0 * spread - 3.0)).unsqueeze(1)
    elif name == "near_degenerate":
        up = torch.nn.functional.normalize(center.float().double() - eye.float().double(), dim=1) + 1e-2 * extra
    elif name == "close":
        center = eye.float().double() + 1e-3 * extra
    elif name != "plain":
        raise KeyError(name)
    return {k: v.float().contiguous() for k, v in (("eye", eye), ("center", center), ("up", up), ("fov", fov),
                                                   ("near", near), ("far", far))}


def degenerate_batch(edit, at=300):
    """600 plain cameras; camera `at` alone degenerate: eye == center (bit 0), up parallel to the gaze (bit 1), a NaN eye
    component (both), or None for the batch as it is."""
    cam = {k: v.clone() for k, v in family("plain", SIZE).items()}
    if edit == "eye_is_center":
        cam["center"][at] = cam["eye"][at]
    elif edit == "up_along_gaze":
        cam["center"][at] = cam["eye"][at]
        cam["center"][at, 2] -= 2.0             # the gaze is (0, 0, -1) exactly
        cam["up"][at] = torch.tensor([0.0, 0.0, 3.0])
    elif edit == "nan_eye":
        cam["eye"][at, 1] = float("nan")
    else:
        assert edit is None
    return cam


def weights_for(batch, seed=SEED):
    """Random upstream [B,4,4] for the matrix, float32."""
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randn(batch, 4, 4, generator=g, dtype=torch.float64).float()


def prefix(cam, batch):
    return {k: v[:batch].contiguous() for k, v in cam.items()}


def lengths(cam, dtype=torch.float64):
    """-> (f_len [B], s_len [B]): |center - eye| and |gaze x up|, the two quantities look_at holds to the cut-off."""
    eye, center, up = (cam[k].to(dtype) for k in INPUTS)
    forward = center - eye
    f_len = torch.linalg.norm(forward, dim=1)
    s_len = torch.linalg.norm(torch.cross(forward / f_len.unsqueeze(1), up, dim=-1), dim=1)
    return f_len, s_len


def flags(cam, dtype=torch.float64):
    """int [B]: bit 0 eye ~ center, bit 1 up ~ gaze (or up degenerate), look_at's two assertions per camera.  Written as
    "not greater than", so a NaN raises both; the second is judged only where the first leaves a gaze to judge it by
    (look_at stops at its first assertion: with eye == center the gaze is 0 / 0 whatever the up vector)."""
    f_len, s_len = lengths(cam, dtype)
    return (~(f_len > CUTOFF)).int() + 2 * (~(s_len > CUTOFF) & ~(f_len <= CUTOFF)).int()


def _matrix(eye, center, up, fov, near, far, aspect):
    return torch.matmul(camera_utils.perspective(aspect, fov, near, far), camera_utils.look_at(eye, center, up))


def transforms(eye, center, up, fov, near, far, aspect, dtype, weights=None, fov_grad=False):
    """perspective @ look_at in `dtype` on the host -> (matrix [B,4,4], gradients).  gradients: None without
    `weights` [B,4,4], else the dict of d sum(matrix * weights) / d eye, center, up (and fov with `fov_grad`)."""
    leaves = {k: v.detach().cpu().to(dtype).clone().requires_grad_(weights is not None)
              for k, v in (("eye", eye), ("center", center), ("up", up))}
    fov = fov.detach().cpu().to(dtype).clone().requires_grad_(weights is not None and fov_grad)
    m = _matrix(leaves["eye"], leaves["center"], leaves["up"], fov, near.detach().cpu().to(dtype),
                far.detach().cpu().to(dtype), aspect)
    if weights is None:
        return m.detach(), None
    names = list(INPUTS) + (["fov"] if fov_grad else [])
    wanted = [leaves[k] for k in INPUTS] + ([fov] if fov_grad else [])
    grads = torch.autograd.grad((m * weights.detach().cpu().to(dtype)).sum(), wanted)
    return m.detach(), dict(zip(names, (g.detach() for g in grads)))


def jacobian(eye, center, up, fov, near, far, aspect):
    """float64 d transforms[b] / d (eye, center, up)[b] -> [B,16,9] (row-major matrix entries; eye, center, up)."""
    leaves = [t.detach().cpu().double().clone().requires_grad_(True) for t in (eye, center, up)]
    f64 = lambda t: t.detach().cpu().double()
    m = _matrix(*leaves, f64(fov), f64(near), f64(far), aspect).reshape(-1, 16)
    rows = []
    for i in range(16):    # cameras are independent: the sum over b of entry i separates by camera
        rows.append(torch.cat(torch.autograd.grad(m[:, i].sum(), leaves, retain_graph=True), dim=1))
    return torch.stack(rows, dim=1)


def per_camera_error(got, want):
    """[B]: max|got[b] - want[b]| / max|want[b]|."""
    B = want.shape[0]
    got, want = got.detach().cpu().double().reshape(B, -1), want.double().reshape(B, -1)
    return (got - want).abs().max(1).values / want.abs().max(1).values


def evaluate(cam, weights, aspect=ASPECT, fov_grad=False):
    """-> (truth, r): truth = {"matrix", "eye", "center", "up"[, "fov"]} in float64, r = the float32 restatement's
    worst per-camera relative error by the same names."""
    args = [cam[k] for k in ("eye", "center", "up", "fov", "near", "far")]
    m64, g64 = transforms(*args, aspect, torch.float64, weights, fov_grad)
    m32, g32 = transforms(*args, aspect, torch.float32, weights, fov_grad)
    truth = dict(g64, matrix=m64)
    got32 = dict(g32, matrix=m32)
    return truth, {k: float(per_camera_error(got32[k], truth[k]).max()) for k in truth}


@functools.lru_cache(maxsize=None)
def family_truth(name, fov_grad=False):
    """-> (cameras, weights, truth, r) of the whole family (SIZE cameras), computed once."""
    cam, w = family(name, SIZE), weights_for(SIZE)
    truth, r = evaluate(cam, w, fov_grad=fov_grad)
    return cam, w, truth, r


def compare(label, got, truth, r, batch=None, k=K):
    """got / truth: dicts by tensor name ([B,...]; the truth is cut to `batch` cameras), r: the family's ref_err.
    Prints the worst per-camera error over r per tensor -> (list of violations, {tensor: ratio})."""
    over, ratios = [], {}
    for name, g in got.items():
        want = truth[name] if batch is None else truth[name][:batch]
        B = want.shape[0]
        g = g.detach().cpu().double().reshape(B, -1)
        w = want.double().reshape(B, -1)
        scale = w.abs().max(1).values
        err = (g - w).abs().max(1).values
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
        bound = k * r[name] * scale + FLOOR * float(w.abs().max())
        ratios[name] = float((err / scale).max()) / max(r[name], 1e-300)
        worst = int((err / bound).argmax())
        print("%-32s %-7s got_err %.3g  ref_err %.3g  ratio %.3g  worst camera %d at %.3g of its bound" % (
            label, name, float((err / scale).max()), r[name], ratios[name], worst, float(err[worst] / bound[worst])))
        if not bool((err <= bound).all()):
            over.append("%s %s: camera %d off by %.3g, allowed %.3g" % (label, name, worst, float(err[worst]),
                                                                        float(bound[worst])))
    return over, ratios
