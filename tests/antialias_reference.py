"""Restatement of mesh_renderer.antialias, written from its specification ("Silhouette
antialiasing"), not from the kernel.

The discrete decisions -- coverage, front pixel, edge functions, exit edge, silhouette side -- are evaluated
in numpy float32, un-fused, in the specified order, so the set of blended pairs is the kernel's bit for bit.
Blend values and gradients come in two spellings that say the same thing:

  antialias()        float64 torch with autograd: the crossing parameter t takes the float32 value the decision
                     produced and the float64 slope (row . P_c) / D with respect to the clip coordinates of the
                     exit edge's two vertices, P_c = f + t (g - f) the crossing point of that decided t
  pair_gradients()   rule 8 literally, pair by pair: dL/dt, D = row . (P_f - P_g), P_c = f + t (g - f) with the
                     float32 t, dt/dv_a = s (v_b x P_c) / D, dt/dv_b = s (P_c x v_a) / D -- in float64 the truth,
                     with a noise scale next to it; in float32, in the documented evaluation order, the
                     restatement whose distance from the truth calibrates the bound of the GPU tests
  autograd_slopes()  the derivative of the quotient e(f) / (e(f) - e(g)) itself, by torch

Where 0 < t < 1 the literal formula AT THE FLOAT64 QUOTIENT is the quotient's derivative (to 1e-12; asserted in
tests/test_antialias_truth_host.py); at the decided float32 t it differs by that t's rounding, a fraction of a pixel
in P_c, which the kernel carries too, so the truth carries it.  Where rule 5 clamped t (t == 0 or t == 1: only a
G-buffer that does not belong to `clip` gets there, the rasterizer's own has e(f) >= 0) the derivative of the
unclamped quotient is NOT what rule 8 says: P_c is the crossing point of the CLAMPED t, an end of the segment, and the
slope is the literal formula's there.  antialias() and pair_gradients() agree on every pair.  blend() /
blend_backward() are the literal image side, with noise scales.
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
    exit-edge vertex indices, t (float32), s (the adjugate's sign), horizontal.  Also the pair mask [B,H,W] u8
    (bit k of a pixel: its pair with the left / right / down / up neighbour blended into it).
    pairs["candidates"]: every pair rule 2 looks at (b, its two pixels a / b) with blended, half (everything but
    t != 0.5 holds) and equal_z (rule 3 came down to the ids)."""
    ids, bary, z = np.asarray(ids), np.asarray(bary, dtype=F32), np.asarray(z, dtype=F32)
    clip, tris, opp = np.asarray(clip, dtype=F32), np.asarray(triangles), np.asarray(opposite)
    B, H, W = ids.shape
    V, T = clip.shape[1], tris.shape[0]
    cov = (ids != 0) | (((bary[..., 0] + bary[..., 1]) + bary[..., 2]) >= F32(0.9))
    cx, cy = _centres(W, F32(0.5 * W)), _centres(H, F32(0.5 * H))
    out = {k: [] for k in ("b", "fy", "fx", "gy", "gx", "my", "mx", "oy", "ox", "bit", "va", "vb", "t", "mod_f", "s",
                           "horizontal")}
    cand = {k: [] for k in ("b", "ay", "ax", "by", "bx", "blended", "half", "equal_z")}
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
        half = ok & ~interior & (t == F32(0.5))
        ok &= ~interior & (t != F32(0.5))
        for name, v in (("b", bb), ("ay", ay), ("ax", ax), ("by", by), ("bx", bx), ("blended", ok), ("half", half),
                        ("equal_z", (ca == cb) & (za == zb))):
            cand[name].append(v)
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
                        ("t", t[sel]), ("mod_f", mod_f), ("s", np.where(det[sel] < 0, F32(-1), F32(1))),
                        ("horizontal", np.full(len(sel), horizontal))):
            out[name].append(v)
        np.bitwise_or.at(mask, (bb[sel], my, mx), (1 << bit).astype(np.uint8))
    pairs = {k: np.concatenate(v) for k, v in out.items()}
    pairs["centres"] = (cx, cy)
    pairs["candidates"] = {k: np.concatenate(v) for k, v in cand.items()}
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
    t32 = f64(pairs["t"])
    # rule 8: d t / d row = P_c / D at the crossing point of the DECIDED t, P_c = f + t (g - f).  Where 0 < t < 1 this
    # is the slope of the quotient e(f) / (e(f) - e(g)) itself (at the float64 quotient to 1e-12; t's float32 rounding
    # moves P_c by that much of a pixel); where rule 5 clamped t it is the same expression at the end of the segment
    Pc = Pf + t32[:, None] * (Pg - Pf)
    slope = (row * Pc).sum(1) / (ef - eg).detach()
    t = t32 + (slope - slope.detach())                              # the float32 decision's value, float64 slope
    mod_f = torch.as_tensor(pairs["mod_f"])
    wgt = torch.where(mod_f, 0.5 - t, t - 0.5)
    contrib = wgt[:, None] * (flat[o_i] - flat[m_i])
    out = flat.index_add(0, m_i, contrib)
    return out.reshape(B, H, W, C)


# ---- rule 8 spelled out, with noise scales ---------------------------------------------------------------------------
U32 = 2.0 ** -24


def _np(a, dtype):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.astype(dtype)


def _weights(pairs, dtype):
    t = pairs["t"].astype(dtype)
    half = np.dtype(dtype).type(0.5)
    return np.where(pairs["mod_f"], half - t, t - half)


def pair_terms(image, dout, clip, pairs, dtype=np.float64, t=None):
    """Rule 8 for every pair of `pairs`, in `dtype`, each operation in the order the rule (and the kernel's comments)
    give it -> dict of arrays over pairs:
      dldt [n]        sum_ch dout[m] (c_f - c_g), channels in order;   dldt_abs: the same sum of absolute values
      D [n]           row . (P_f - P_g): the one non-zero component of the sign-normalised exit row s (v_a x v_b)
                      times the centre difference;   cond_d = (|p q| + |r s|) |delta| / |D|, how many of its own
                      roundings D carries (the row component is a difference of two products)
      slope_a, slope_b [n,3]   dt/d(x, y, w) of the edge's two vertices: s (v_b x P_c) / D and s (P_c x v_a) / D
      ga, gb [n,3]    (dldt * (s / D)) * cross, as evaluated;   na, nb: their noise scales
    P_c = f + t (g - f) with the float32 t of decide() (or the t given: the host test passes the float64 quotient)."""
    image, dout, clip = _np(image, dtype), _np(dout, dtype), _np(clip, dtype)
    b, cx, cy = pairs["b"], pairs["centres"][0].astype(dtype), pairs["centres"][1].astype(dtype)
    n, C = len(b), image.shape[3]
    cf, cg = image[b, pairs["fy"], pairs["fx"]], image[b, pairs["gy"], pairs["gx"]]
    dm = dout[b, pairs["my"], pairs["mx"]]
    dldt, dldt_abs = np.zeros(n, dtype), np.zeros(n, dtype)
    for c in range(C):
        term = dm[:, c] * (cf[:, c] - cg[:, c])
        dldt, dldt_abs = dldt + term, dldt_abs + np.abs(term)
    va, vb = clip[b, pairs["va"]], clip[b, pairs["vb"]]
    ax, ay, aw, bx, by, bw = va[:, 0], va[:, 1], va[:, 3], vb[:, 0], vb[:, 1], vb[:, 3]
    hor, s = pairs["horizontal"], pairs["s"].astype(dtype)
    t = (pairs["t"] if t is None else t).astype(dtype)
    fx, fy, gx, gy = cx[pairs["fx"]], cy[pairs["fy"]], cx[pairs["gx"]], cy[pairs["gy"]]
    # the adjugate row of the edge joining a and b is v_a x v_b = (ya wb - wa yb, xb wa - wb xa, ..): SURVEY.md Appendix A
    p1, p2 = np.where(hor, ay * bw, bx * aw), np.where(hor, aw * by, bw * ax)
    delta = np.where(hor, fx - gx, fy - gy)
    with np.errstate(divide="ignore", invalid="ignore"):
        D = (s * (p1 - p2)) * delta
        inv_d = s / D
        cond_d = (np.abs(p1) + np.abs(p2)) * np.abs(delta) / np.abs(D)
        px, py = fx + t * (gx - fx), fy + t * (gy - fy)
        pax, pay = np.abs(fx) + np.abs(t * (gx - fx)), np.abs(fy) + np.abs(t * (gy - fy))
        cross_a = np.stack([by - bw * py, bw * px - bx, bx * py - by * px], 1)
        cross_b = np.stack([py * aw - ay, ax - px * aw, px * ay - py * ax], 1)
        abs_a = np.stack([np.abs(by) + np.abs(bw) * pay, np.abs(bw) * pax + np.abs(bx),
                          np.abs(bx) * pay + np.abs(by) * pax], 1)
        abs_b = np.stack([pay * np.abs(aw) + np.abs(ay), np.abs(ax) + pax * np.abs(aw),
                          pax * np.abs(ay) + pay * np.abs(ax)], 1)
        sc = dldt * inv_d
        scn = dldt_abs * np.abs(inv_d) * (1.0 + cond_d)
        return {"dldt": dldt, "dldt_abs": dldt_abs, "D": D, "cond_d": cond_d,
                "slope_a": inv_d[:, None] * cross_a, "slope_b": inv_d[:, None] * cross_b,
                "ga": sc[:, None] * cross_a, "gb": sc[:, None] * cross_b,
                "na": scn[:, None] * abs_a, "nb": scn[:, None] * abs_b}


def pair_gradients(image, dout, clip, pairs, dtype=np.float64):
    """-> (dclip, noise) [B,V,4] float64: rule 8 evaluated in `dtype` (pair_terms) and summed per vertex in pair order,
    and the noise scale of every element: the sum over the vertex's pairs of the absolute values of the terms, times
    one plus D's conditioning.  dtype=float64: the truth.  dtype=float32: the float32 restatement."""
    clip_shape = tuple(clip.shape)
    p = pair_terms(image, dout, clip, pairs, dtype)
    dclip, noise = np.zeros(clip_shape, dtype), np.zeros(clip_shape, np.float64)
    b = pairs["b"]
    for v, g, nz in ((pairs["va"], p["ga"], p["na"]), (pairs["vb"], p["gb"], p["nb"])):
        for i, col in enumerate((0, 1, 3)):                           # no gradient to clip z
            np.add.at(dclip[..., col], (b, v), g[:, i])
            np.add.at(noise[..., col], (b, v), nz[:, i].astype(np.float64))
    return dclip.astype(np.float64), noise


def autograd_slopes(clip, pairs):
    """dt/d(x, y, w) of both vertices of every pair from the autograd spelling (the quotient e(f) / (e(f) - e(g)) in
    float64, differentiated by torch) -> (slope_a, slope_b [n,3], the float64 quotient [n]).  Only meaningful where
    0 < t < 1."""
    clip = torch.as_tensor(_np(clip, np.float64))
    b = torch.as_tensor(pairs["b"], dtype=torch.int64)
    n = len(b)
    cx, cy = pairs["centres"]
    xyw = lambda k: clip[b, torch.as_tensor(pairs[k], dtype=torch.int64)][:, [0, 1, 3]].clone().requires_grad_(True)
    A, Bv = xyw("va"), xyw("vb")
    f64 = lambda v: torch.as_tensor(v.astype(np.float64))
    Pf = torch.stack([f64(cx[pairs["fx"]]), f64(cy[pairs["fy"]]), torch.ones(n, dtype=torch.float64)], 1)
    Pg = torch.stack([f64(cx[pairs["gx"]]), f64(cy[pairs["gy"]]), torch.ones(n, dtype=torch.float64)], 1)
    row = torch.cross(A, Bv, dim=1)
    ef, eg = (row * Pf).sum(1), (row * Pg).sum(1)
    t64 = ef / (ef - eg)
    t64.sum().backward()
    return A.grad.numpy(), Bv.grad.numpy(), t64.detach().numpy()


def blend(image, pairs, dtype=np.float64):
    """Rule 7 in `dtype`, each pixel adding its pairs in the order left, right, down, up -> (out, noise) [B,H,W,C]
    float64, noise = |c_p| + sum over the pairs that modify p of |w| (|c_o| + |c_p|)."""
    image = _np(image, dtype)
    out, noise = image.copy(), np.abs(image).astype(np.float64)
    w, b = _weights(pairs, dtype), pairs["b"]
    for k in range(4):
        sel = pairs["bit"] == k
        m, o = (b[sel], pairs["my"][sel], pairs["mx"][sel]), (b[sel], pairs["oy"][sel], pairs["ox"][sel])
        out[m] = out[m] + w[sel, None] * (image[o] - image[m])        # at most one pair per pixel and direction
        noise[m] += np.abs(w[sel, None]).astype(np.float64) * (np.abs(image[o]) + np.abs(image[m]))
    return out.astype(np.float64), noise


def blend_backward(dout, pairs, dtype=np.float64):
    """d image of rule 7 in `dtype`, gathered per pixel over its four directions in order: the modified pixel keeps
    dout (1 - w), the other pixel gains w dout[m] -> (dimage, noise) [B,H,W,C] float64, noise = |d_p| + sum |w d_m|
    over every pair p belongs to."""
    dout = _np(dout, dtype)
    d, noise = dout.copy(), np.abs(dout).astype(np.float64)
    w, b = _weights(pairs, dtype), pairs["b"]
    for k in range(4):
        for as_modified in (True, False):
            sel = pairs["bit"] == k if as_modified else (pairs["bit"] ^ 1) == k
            m, o = (b[sel], pairs["my"][sel], pairs["mx"][sel]), (b[sel], pairs["oy"][sel], pairs["ox"][sel])
            term = w[sel, None] * dout[m]
            if as_modified:
                d[m] = d[m] - term
                noise[m] += np.abs(term)
            else:
                d[o] = d[o] + term
                noise[o] += np.abs(term)
    return d.astype(np.float64), noise


def excess(got, truth, noise, K, extra=0.0, floor=1e-7):
    """max over elements of |got - truth| / (K 2^-24 noise + extra + floor max|truth|); a NaN or an infinity in
    `got` where the truth is finite counts as infinite.  <= 1: inside the bound."""
    got = _np(got, np.float64)
    if got.size == 0:
        return 0.0
    allowed = K * U32 * noise + extra + floor * float(np.abs(truth).max())
    err = np.where(np.isfinite(got) | ~np.isfinite(truth), np.abs(got - truth), np.inf)
    ok = np.isfinite(truth) & np.isfinite(allowed)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / allowed)
    return float(r[ok].max()) if ok.any() else 0.0


def r32_ratio(f32, truth, noise):
    """The float32 restatement's distance from the truth in units of 2^-24 noise (largest element; exact zeros of
    both where the noise is zero count as zero)."""
    err = np.abs(np.asarray(f32, np.float64) - truth)
    ok = np.isfinite(truth) & np.isfinite(noise) & (err > 0)
    with np.errstate(divide="ignore"):
        return float((err[ok] / (U32 * noise[ok])).max()) if ok.any() else 0.0
