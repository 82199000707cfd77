"""Independent float64 restatement of spherical-harmonics lighting ("Spherical-harmonics lighting"),
written from the stated formulas; it does not import the package.  Torch float64, so that autograd gives the
reference gradients, on whichever device the inputs live."""
import math

import numpy as np
import torch

# Y_k(x, y, z) for a unit normal, in the documented order
C0 = 0.282094791773878
C1 = 0.488602511902920
C2 = 1.092548430592079
C3 = 0.315391565252520
C4 = 0.546274215296040


def basis(n):
    """n [..., 3] (unit) -> Y [..., 9]; works on numpy arrays and torch tensors."""
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    terms = [C0 + 0.0 * x, C1 * y, C1 * z, C1 * x, C2 * x * y, C2 * y * z, C3 * (3.0 * z * z - 1.0), C2 * x * z,
             C4 * (x * x - y * y)]
    if torch.is_tensor(n):
        return torch.stack(terms, -1)
    return np.stack(terms, -1)


def unit(normals):
    """N / max(|N|, 1e-12)."""
    length = torch.linalg.vector_norm(normals, dim=-1, keepdim=True)
    return normals / torch.clamp(length, min=1e-12)


def shade(normals, diffuse, alphas, sh, flip=True):
    """normals, diffuse [B,H,W,3], alphas [B,H,W] or None (any(diffuse >= 0)), sh [B,9,3] -> RGBA [B,H,W,4]
    (float64, differentiable in every input but the mask)."""
    normals, diffuse, sh = normals.double(), diffuse.double(), sh.double()
    if alphas is None:
        alphas = (diffuse >= 0).any(-1).double()
    else:
        alphas = alphas.double()
    Y = basis(unit(normals))                                  # [B,H,W,9]
    E = (Y.unsqueeze(-1) * sh[:, None, None, :, :]).sum(-2)   # [B,H,W,3]
    keep = (alphas > 0.5).unsqueeze(-1).double()
    rgba = torch.cat([diffuse * E * keep, alphas.unsqueeze(-1)], -1)
    return torch.flip(rgba, [1]) if flip else rgba


def dsh_abs_terms(normals, diffuse, alphas, drgba, flip=True):
    """sum over the pixels of |Y_k * g_c * d_c| per [B,9,3] entry: the scale of each dsh sum."""
    normals, diffuse, drgba = normals.double(), diffuse.double(), drgba.double()
    if flip:
        drgba = torch.flip(drgba, [1])
    if alphas is None:
        alphas = (diffuse >= 0).any(-1).double()
    keep = (alphas.double() > 0.5).unsqueeze(-1).double()
    Y = basis(unit(normals)).abs()
    gd = (drgba[..., :3] * diffuse).abs() * keep
    return torch.einsum("bhwk,bhwc->bkc", Y, gd)


def gradients(normals, diffuse, alphas, sh, drgba, flip=True):
    """-> dict of float64 gradients of sum(shade(...) * drgba): normals, diffuse, alphas (or None), sh."""
    leaves = {"normals": normals.double().clone().requires_grad_(True),
              "diffuse": diffuse.double().clone().requires_grad_(True),
              "sh": sh.double().clone().requires_grad_(True)}
    a = None
    if alphas is not None:
        a = leaves["alphas"] = alphas.double().clone().requires_grad_(True)
    out = shade(leaves["normals"], leaves["diffuse"], a, leaves["sh"], flip)
    (out * drgba.double()).sum().backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads.setdefault("alphas", None)
    return grads


def sphere_quadrature(n_theta=24, n_phi=48):
    """Points and weights integrating exactly any polynomial of degree < 2 n_theta on the unit sphere:
    Gauss-Legendre in cos(theta) times the trapezoid rule in phi."""
    u, w = np.polynomial.legendre.leggauss(n_theta)
    phi = np.arange(n_phi) * (2.0 * math.pi / n_phi)
    s = np.sqrt(1.0 - u * u)
    pts = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)), np.outer(u, np.ones_like(phi))], -1)
    weights = np.outer(w, np.full(n_phi, 2.0 * math.pi / n_phi))
    return pts.reshape(-1, 3), weights.reshape(-1)
