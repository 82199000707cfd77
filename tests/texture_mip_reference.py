"""An independent restatement of mipmapped trilinear texture sampling and of the screen-space attribute
derivatives ("Texture mapping").

The pyramid is binary32 in the stated order, fl(fl(fl(a + b) + fl(c + d)) * 0.25f); the tap decision per level is
texture_reference's (binary32); everything after that is float64.  Works on CPU or device tensors.  The derivative
restatement is numpy: U, e and s in float32 in the oracle's order, the rest in float64 (or all float32, to measure
what the formula loses in single precision).
"""
import numpy as np
import torch

import texture_reference as tr


def _tz(n):
    return (n & -n).bit_length() - 1


def levels(Ht, Wt, max_mip_level=None):
    l = min(_tz(Ht), _tz(Wt))
    return 1 + (l if max_mip_level is None else min(l, max_mip_level))


def pyramid(tex, max_mip_level=None):
    """tex [..., Ht, Wt, C] float32 -> [level 0, level 1, ...], float32, each the 2 x 2 box filter of the one before,
    operation by operation in tex's dtype (a float64 texture gives the unrounded pyramid: for difference quotients)."""
    out = [tex]
    for _ in range(1, levels(tex.shape[-3], tex.shape[-2], max_mip_level)):
        t = out[-1]
        a, b = t[..., 0::2, 0::2, :], t[..., 0::2, 1::2, :]
        c, d = t[..., 1::2, 0::2, :], t[..., 1::2, 1::2, :]
        out.append(((a + b) + (c + d)) * torch.tensor(0.25, dtype=tex.dtype))
    return out


def lod(uv_da, Ht, Wt, L):
    """uv_da [B,H,W,4] float32 (du/dX, du/dY, dv/dX, dv/dY) -> (l0 long, f float64): lod = 0.5 log2(max(ax^2, ay^2)),
    a NaN taken as 0, clamped to [0, L - 1]."""
    d = uv_da.double()
    ax2 = (d[..., 0] * Wt) ** 2 + (d[..., 2] * Ht) ** 2
    ay2 = (d[..., 1] * Wt) ** 2 + (d[..., 3] * Ht) ** 2
    lam = 0.5 * torch.log2(torch.maximum(ax2, ay2))          # maximum propagates a NaN
    lam = torch.where(torch.isnan(lam), torch.zeros_like(lam), lam).clamp(0.0, float(L - 1))
    l0 = torch.floor(lam)
    return l0.long(), lam - l0


def _level_weights(l0, f, valid, l):
    """-> (weight of level l per pixel, float64; whether the pixel reads level l at all)."""
    lower = valid & (l0 == l)
    upper = valid & (l0 + 1 == l) & (f > 0)
    zero = torch.zeros_like(f)
    return torch.where(lower, 1 - f, zero) + torch.where(upper, f, zero), lower | upper


def fold(grad_levels):
    """[d level 0, d level 1, ...] (float64, [B,Hl,Wl,C]) -> d level 0 after dlevel_l[i,j] += 0.25 dlevel_{l+1}[i/2,j/2],
    coarsest first."""
    acc = grad_levels[-1]
    for g in reversed(grad_levels[:-1]):
        acc = g + 0.25 * acc.repeat_interleave(2, 1).repeat_interleave(2, 2)
    return acc


def sample(tex, uv, uv_da, mask=None, boundary="wrap", max_mip_level=None, dout=None):
    """tex [Ht,Wt,C] or [B,Ht,Wt,C] float32, uv [B,H,W,2], uv_da [B,H,W,4] -> value [B,H,W,C] float64.  With dout also
    the gradients: -> (value, dtex (tex's shape), duv [B,H,W,2], abs_sum (tex's shape): the same scatter and fold
    applied to |dout| with both level weights replaced by 1, the scale of dtex's rounding)."""
    B = uv.shape[0]
    Ht, Wt, C = tex.shape[-3:]
    pyr = pyramid(tex, max_mip_level)
    L = len(pyr)
    valid = tr.taps(uv, Ht, Wt, mask, boundary)[0]                      # the skip rule, at level 0
    l0, f = lod(uv_da, Ht, Wt, L)
    bi = torch.arange(B, device=uv.device).view(B, 1, 1).expand(valid.shape)
    value = torch.zeros(*valid.shape, C, dtype=torch.float64, device=uv.device)
    if dout is not None:
        g = torch.where(valid.unsqueeze(3), dout.double(), torch.zeros_like(value))
        du = torch.zeros(valid.shape, dtype=torch.float64, device=uv.device)
        dv = torch.zeros_like(du)
        dlev, alev = [], []
    for l, level in enumerate(pyr):
        Hl, Wl = level.shape[-3:-1]
        wl, reads = _level_weights(l0, f, valid, l)
        t = tr._batched(level, B)
        _, fx, fy, tp = tr.taps(uv, Hl, Wl, None, boundary)
        fx, fy = torch.where(valid, fx, torch.zeros_like(fx)), torch.where(valid, fy, torch.zeros_like(fy))
        tp = [(torch.where(valid, r, torch.zeros_like(r)), torch.where(valid, c, torch.zeros_like(c))) for r, c in tp]
        w = tr._weights(fx, fy)
        vals = [t[bi, r, c] for r, c in tp]
        value = value + wl.unsqueeze(3) * sum(wk.unsqueeze(3) * vk for wk, vk in zip(w, vals))
        if dout is None:
            continue
        t00, t01, t10, t11 = vals
        du = du + wl * Wl * (g * ((1 - fy).unsqueeze(3) * (t01 - t00) + fy.unsqueeze(3) * (t11 - t10))).sum(3)
        dv = dv + wl * Hl * (g * ((1 - fx).unsqueeze(3) * (t10 - t00) + fx.unsqueeze(3) * (t11 - t01))).sum(3)
        dl = torch.zeros(B * Hl * Wl, C, dtype=torch.float64, device=uv.device)
        al = torch.zeros_like(dl)
        for wk, (r, c) in zip(w, tp):
            flat = ((bi * Hl + r) * Wl + c).reshape(-1)
            dl.index_add_(0, flat, ((wl * wk).unsqueeze(3) * g).reshape(-1, C))
            al.index_add_(0, flat, ((reads.double() * wk).unsqueeze(3) * g.abs()).reshape(-1, C))
        dlev.append(dl.view(B, Hl, Wl, C))
        alev.append(al.view(B, Hl, Wl, C))
    if dout is None:
        return value
    dtex, abs_sum = fold(dlev), fold(alev)
    if tex.dim() == 3:
        dtex, abs_sum = dtex.sum(0), abs_sum.sum(0)
    return value, dtex, torch.stack([du, dv], 3), abs_sum


# ---- screen-space attribute derivatives ---------------------------------------------------------------------------
def adjugate_signed(x, y, w, dtype):
    """Rows = edge functions of the triangle with corner coordinates x, y, w ([..., 3] each), sign-corrected; in
    `dtype`, operation by operation in the oracle's order (oracle/mr_oracle.c: adjugate_signed)."""
    x, y, w = (v.astype(dtype) for v in (x, y, w))
    a11, a12, a13 = x[..., 0], x[..., 1], x[..., 2]
    a21, a22, a23 = y[..., 0], y[..., 1], y[..., 2]
    a31, a32, a33 = w[..., 0], w[..., 1], w[..., 2]
    u = [a22 * a33 - a32 * a23, a13 * a32 - a33 * a12, a12 * a23 - a22 * a13,
         a23 * a31 - a33 * a21, a11 * a33 - a31 * a13, a13 * a21 - a23 * a11,
         a21 * a32 - a31 * a22, a12 * a31 - a32 * a11, a11 * a22 - a21 * a12]
    det = (a11 * u[0] + a12 * u[3]) + a13 * u[6]
    sign = np.where(det < 0, -1, 1).astype(dtype)
    return [sign * v for v in u]


def pixel_centres(W, H):
    """NDC of the pixel centres, as the rasterizer forms them: binary64 expression, rounded once."""
    hw, hh = np.float32(0.5 * W), np.float32(0.5 * H)
    px = ((np.arange(W, dtype=np.float64) + 0.5) / np.float64(hw) - 1.0).astype(np.float32)
    py = ((np.arange(H, dtype=np.float64) + 0.5) / np.float64(hh) - 1.0).astype(np.float32)
    return px, py


def interpolate64(x, y, w, a, px, py):
    """Perspective-correct interpolation of corner values a [3] at the NDC point (px, py), all float64."""
    u = adjugate_signed(np.asarray(x), np.asarray(y), np.asarray(w), np.float64)
    e = [u[3 * i] * px + u[3 * i + 1] * py + u[3 * i + 2] for i in range(3)]
    s = e[0] + e[1] + e[2]
    return sum(e[i] / s * a[i] for i in range(3))


def attribute_derivatives(ids, bary, clip, triangles, attributes, attribute_triangles=None, all_float32=False):
    """numpy: ids [B,H,W] int32, bary [B,H,W,3], clip [B,V,4], triangles [T,3], attributes [B,Va,A] ->
    (deriv [B,H,W,A,2], scale [B,H,W,A,2], covered [B,H,W] bool).  U, e and s are float32 in the oracle's order; the
    rest is float64, or float32 with all_float32.  scale = (2/W) sum_i |a_i| (|U[3i]| + |b_i| sum_j |U[3j]|) / s
    (likewise for Y): what one rounding of each term is relative to."""
    B, H, W = ids.shape
    T = triangles.shape[0]
    f32 = np.float32
    bary = bary.astype(f32)
    covered = ((f32(2) * bary[..., 0] + f32(2) * bary[..., 1]) + f32(2) * bary[..., 2] > 0) & (ids >= 0) & (ids < T)
    t = np.where(covered, ids, 0)
    bidx = np.arange(B).reshape(B, 1, 1, 1)
    corners = clip.astype(f32)[bidx, triangles[t]]                       # [B,H,W,3,4]
    u = adjugate_signed(corners[..., 0], corners[..., 1], corners[..., 3], f32)
    px, py = pixel_centres(W, H)
    px, py = px.reshape(1, 1, W), py.reshape(1, H, 1)
    e = [(u[3 * i] * px + u[3 * i + 1] * py) + u[3 * i + 2] for i in range(3)]
    s = (e[0] + e[1]) + e[2]
    assert s.dtype == f32
    ft = f32 if all_float32 else np.float64
    u = [v.astype(ft) for v in u]
    s, b = s.astype(ft), bary.astype(ft)
    a = attributes.astype(ft)[bidx, (attribute_triangles if attribute_triangles is not None else triangles)[t]]
    deriv = np.zeros((B, H, W, a.shape[-1], 2), ft)
    scale = np.zeros_like(deriv)
    with np.errstate(all="ignore"):
        for axis, step in ((0, ft(2) / ft(W)), (1, ft(2) / ft(H))):
            col = [u[axis], u[3 + axis], u[6 + axis]]
            total = (col[0] + col[1]) + col[2]
            abs_total = (np.abs(col[0]) + np.abs(col[1])) + np.abs(col[2])
            for i in range(3):
                ai = a[..., i, :]
                deriv[..., axis] += ai * ((col[i] - b[..., i] * total) / s * step)[..., None]
                scale[..., axis] += np.abs(ai) * ((np.abs(col[i]) + np.abs(b[..., i]) * abs_total) / s * step)[..., None]
    deriv[~covered] = 0
    scale[~covered] = 0
    return deriv, scale, covered
