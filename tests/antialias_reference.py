"""Restatement of mesh_renderer.antialias, written from its specification ("Silhouette
antialiasing"), not from the kernel.

The discrete decisions -- coverage, front pixel, edge functions, exit edge, silhouette side -- are evaluated
in numpy float32, un-fused, in the specified order, so the set of blended pairs is the kernel's bit for bit.
Blend values and gradients are float64 torch with autograd: the crossing parameter t takes the float32
value the decision produced and the float64 derivative of e(f) / (e(f) - e(g)) with respect to the clip
coordinates of the exit edge's two vertices.
"""
import numpy as np
import torch

LEFT, RIGHT, DOWN, UP = 0, 1, 2, 3
F32 = np.float32


def topology(triangles, vertex_count):
    """opposite [T,3] by a plain dictionary walk (the specification of antialias_topology)."""
    tris = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    edges = {}
    for t, tri in enumerate(tris):
        for k in range(3):
            a, b = tri[(k + 1) % 3], tri[(k + 2) % 3]
            edges.setdefault((min(a, b), max(a, b)), []).append((t, k))
    opp = np.full(tris.shape, -1, dtype=np.int32)
    for (lo, hi), users in edges.items():
        for t, k in users:
            if lo == hi or len(users) > 2:
                opp[t, k] = -2
            elif len(users) == 2:
                t2, k2 = users[0] if users[1] == (t, k) else users[1]
                d = tris[t2, k2]
                opp[t, k] = -2 if d in (lo, hi) else d
    return opp


def _centres(n, half):
    return ((np.arange(n, dtype=np.float64) + 0.5) / np.float64(half) - 1.0).astype(F32)


def decide(ids, bary, z, clip, triangles, opposite):
    """Every blended pair, as arrays over pairs: b, f / g pixel (iy, ix), modified pixel, direction bits,
    exit-edge vertex indices, t (float32).  Also the pair mask [B,H,W] u8 (bit k of a pixel: its pair with
    the left / right / down / up neighbour blended into it)."""
    ids, bary, z = np.asarray(ids), np.asarray(bary, dtype=F32), np.asarray(z, dtype=F32)
    clip, tris, opp = np.asarray(clip, dtype=F32), np.asarray(triangles), np.asarray(opposite)
    B, H, W = ids.shape
    V, T = clip.shape[1], tris.shape[0]
    cov = (ids != 0) | (((bary[..., 0] + bary[..., 1]) + bary[..., 2]) >= F32(0.9))
    cx, cy = _centres(W, F32(0.5 * W)), _centres(H, F32(0.5 * H))
    out = {k: [] for k in ("b", "fy", "fx", "gy", "gx", "my", "mx", "oy", "ox", "bit", "va", "vb", "t", "mod_f")}
    mask = np.zeros((B, H, W), dtype=np.uint8)
    for horizontal in (True, False):
        if horizontal:
            bb, ay, ax = np.meshgrid(np.arange(B), np.arange(H), np.arange(W - 1), indexing="ij")
            by, bx = ay, ax + 1
        else:
            bb, ay, ax = np.meshgrid(np.arange(B), np.arange(H - 1), np.arange(W), indexing="ij")
            by, bx = ay + 1, ax
        bb, ay, ax, by, bx = (v.reshape(-1) for v in (bb, ay, ax, by, bx))
        ida, idb = ids[bb, ay, ax], ids[bb, by, bx]
        ca, cb = cov[bb, ay, ax], cov[bb, by, bx]
        keep = (ida != idb) | (ca != cb)
        bb, ay, ax, by, bx, ida, idb, ca, cb = (v[keep] for v in (bb, ay, ax, by, bx, ida, idb, ca, cb))
        za, zb = z[bb, ay, ax], z[bb, by, bx]
        f_is_a = np.where(ca != cb, ca, (za < zb) | ((za == zb) & (ida > idb)))
        F = np.where(f_is_a, ida, idb)
        fy, fx = np.where(f_is_a, ay, by), np.where(f_is_a, ax, bx)
        gy, gx = np.where(f_is_a, by, ay), np.where(f_is_a, bx, ax)
        ok = (F >= 0) & (F < T)
        Fc = np.where(ok, F, 0)
        vi = tris[Fc] if T > 0 else np.zeros((len(F), 3), dtype=np.int64)
        ok &= np.all((vi >= 0) & (vi < V), axis=1)
        vi = np.where(ok[:, None], vi, 0)
        P = clip[bb[:, None], vi]                                   # [n,3,4]
        x, y, w = P[..., 0], P[..., 1], P[..., 3]
        ok &= np.all(w > 0, axis=1)
        a11, a12, a13, a21, a22, a23, a31, a32, a33 = (x[:, 0], x[:, 1], x[:, 2], y[:, 0], y[:, 1], y[:, 2],
                                                       w[:, 0], w[:, 1], w[:, 2])
        m = np.stack([a22 * a33 - a32 * a23, a13 * a32 - a33 * a12, a12 * a23 - a22 * a13,
                      a23 * a31 - a33 * a21, a11 * a33 - a31 * a13, a13 * a21 - a23 * a11,
                      a21 * a32 - a31 * a22, a12 * a31 - a32 * a11, a11 * a22 - a21 * a12], axis=1)
        det = (a11 * m[:, 0] + a12 * m[:, 3]) + a13 * m[:, 6]
        m = np.where((det < 0)[:, None], -m, m)
        pfx, pfy, pgx, pgy = cx[fx], cy[fy], cx[gx], cy[gy]
        exit_k = np.full(len(F), -1)
        t = np.zeros(len(F), dtype=F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            for k in range(3):
                ef = (m[:, 3 * k] * pfx + m[:, 3 * k + 1] * pfy) + m[:, 3 * k + 2]
                eg = (m[:, 3 * k] * pgx + m[:, 3 * k + 1] * pgy) + m[:, 3 * k + 2]
                tk = np.fmin(np.fmax(ef / (ef - eg), F32(0)), F32(1))   # fminf / fmaxf: NaN -> the other operand
                take = (eg < 0) & ((exit_k < 0) | (tk < t))
                exit_k = np.where(take, k, exit_k)
                t = np.where(take, tk, t).astype(F32)
        ok &= exit_k >= 0
        k = np.where(exit_k >= 0, exit_k, 0)
        rows = np.arange(len(F))
        d = opp[Fc, k] if T > 0 else np.full(len(F), -1)
        ok &= ~((d >= V))
        dc = np.where((d >= 0) & (d < V), d, 0)
        vd = clip[bb, dc]
        n0, n1, n2 = m[rows, 3 * k], m[rows, 3 * k + 1], m[rows, 3 * k + 2]
        sc = (n0 * x[rows, k] + n1 * y[rows, k]) + n2 * w[rows, k]
        sd = (n0 * vd[:, 0] + n1 * vd[:, 1]) + n2 * vd[:, 3]
        interior = (d >= 0) & (vd[:, 3] > 0) & (((sc > 0) & (sd < 0)) | ((sc < 0) & (sd > 0)))
        ok &= ~interior & (t != F32(0.5))
        sel = np.nonzero(ok)[0]
        mod_f = t[sel] < F32(0.5)
        my, mx = np.where(mod_f, fy[sel], gy[sel]), np.where(mod_f, fx[sel], gx[sel])
        oy, ox = np.where(mod_f, gy[sel], fy[sel]), np.where(mod_f, gx[sel], fx[sel])
        if horizontal:
            bit = np.where(ox > mx, RIGHT, LEFT)
        else:
            bit = np.where(oy > my, UP, DOWN)
        ks = k[sel]
        va = vi[sel, (ks + 1) % 3]
        vb = vi[sel, (ks + 2) % 3]
        for name, v in (("b", bb[sel]), ("fy", fy[sel]), ("fx", fx[sel]), ("gy", gy[sel]), ("gx", gx[sel]),
                        ("my", my), ("mx", mx), ("oy", oy), ("ox", ox), ("bit", bit), ("va", va), ("vb", vb),
                        ("t", t[sel]), ("mod_f", mod_f)):
            out[name].append(v)
        np.bitwise_or.at(mask, (bb[sel], my, mx), (1 << bit).astype(np.uint8))
    pairs = {k: np.concatenate(v) for k, v in out.items()}
    pairs["centres"] = (cx, cy)
    return pairs, mask


def antialias(image, clip, pairs):
    """float64 torch: the antialiased image from `pairs` (decide()), differentiable w.r.t. image [B,H,W,C]
    and clip [B,V,4] (pass float64 leaves to get their gradients)."""
    B, H, W, C = image.shape
    cx, cy = pairs["centres"]
    b = torch.as_tensor(pairs["b"], dtype=torch.int64)
    n = len(b)
    flat = image.reshape(B * H * W, C)
    if n == 0:
        return image + 0.0
    def pix(yk, xk):
        return b * H * W + torch.as_tensor(pairs[yk], dtype=torch.int64) * W + torch.as_tensor(pairs[xk], dtype=torch.int64)
    m_i, o_i = pix("my", "mx"), pix("oy", "ox")
    va = clip[b, torch.as_tensor(pairs["va"], dtype=torch.int64)]
    vb = clip[b, torch.as_tensor(pairs["vb"], dtype=torch.int64)]
    A = torch.stack([va[:, 0], va[:, 1], va[:, 3]], 1)
    Bv = torch.stack([vb[:, 0], vb[:, 1], vb[:, 3]], 1)
    row = torch.cross(A, Bv, dim=1)                                   # e(p) = row . (px, py, 1), up to sign
    f64 = lambda v: torch.as_tensor(v.astype(np.float64))
    Pf = torch.stack([f64(cx[pairs["fx"]]), f64(cy[pairs["fy"]]), torch.ones(n, dtype=torch.float64)], 1)
    Pg = torch.stack([f64(cx[pairs["gx"]]), f64(cy[pairs["gy"]]), torch.ones(n, dtype=torch.float64)], 1)
    ef, eg = (row * Pf).sum(1), (row * Pg).sum(1)
    t64 = ef / (ef - eg)
    t = f64(pairs["t"]) + (t64 - t64.detach())                      # the float32 decision's value, float64 slope
    mod_f = torch.as_tensor(pairs["mod_f"])
    wgt = torch.where(mod_f, 0.5 - t, t - 0.5)
    contrib = wgt[:, None] * (flat[o_i] - flat[m_i])
    out = flat.index_add(0, m_i, contrib)
    return out.reshape(B, H, W, C)
