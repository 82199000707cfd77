"""float64 restatement of the SSIM loss of mesh_renderer.losses.ssim ("Image losses: SSIM").

image, target: [B, H, W, C] arrays.  Window g[i] ~ exp(-(i - r)^2 / (2 sigma^2)), r = (window_size - 1) / 2, normalised
to sum 1 in float64 and then rounded to float32 (the kernels take float weights); the 2-D window is g x g.  Per channel
and pixel

    mx = G*x  my = G*y  sxx = G*(x x) - mx^2  syy = G*(y y) - my^2  sxy = G*(x y) - mx my
    map = ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sxx + syy + C2)),  C1 = (k1 L)^2, C2 = (k2 L)^2

padding "same": taps outside the image contribute zero, weights not renormalised, the map is H x W; "valid": only the
windows wholly inside, the map is (H - ws + 1) x (W - ws + 1).  The value is the plain mean of the map.  The gradients
are those of upstream * value, by the chain rule through the central moments and the blur's adjoint.
"""
import numpy as np


def window(window_size, sigma):
    i = np.arange(window_size, dtype=np.float64)
    g = np.exp(-(i - (window_size - 1) / 2.0) ** 2 / (2.0 * float(sigma) ** 2))
    return (g / g.sum()).astype(np.float32).astype(np.float64)


def _correlate_axis(x, g, axis, pad):
    """sum_k g[k] x[i + k - pad] along `axis`, zero outside: the output has n + 2 pad - len(g) + 1 entries."""
    width = [(0, 0)] * x.ndim
    width[axis] = (pad, pad)
    xp = np.pad(x, width)
    n = xp.shape[axis] - len(g) + 1
    out = np.zeros(xp.shape[:axis] + (n,) + xp.shape[axis + 1:], dtype=np.float64)
    for k, w in enumerate(g):
        out += w * np.take(xp, np.arange(k, k + n), axis=axis)
    return out


def blur(x, g, padding):
    pad = len(g) // 2 if padding == "same" else 0
    return _correlate_axis(_correlate_axis(x, g, 1, pad), g, 2, pad)


def blur_adjoint(m, g, padding):
    """The transpose of blur(., g, padding), from the map's shape back to the image's (g is symmetric)."""
    pad = len(g) // 2 if padding == "same" else len(g) - 1
    return _correlate_axis(_correlate_axis(m, g[::-1], 1, pad), g[::-1], 2, pad)


def ssim_reference(image, target, window_size=11, sigma=1.5, padding="same", k1=0.01, k2=0.03, data_range=1.0,
                   upstream=1.0):
    """-> {"value", "map", "dimage", "dtarget"} in float64."""
    x, y = np.asarray(image, dtype=np.float64), np.asarray(target, dtype=np.float64)
    g = window(window_size, sigma)
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    mx, my = blur(x, g, padding), blur(y, g, padding)
    sxx = blur(x * x, g, padding) - mx * mx
    syy = blur(y * y, g, padding) - my * my
    sxy = blur(x * y, g, padding) - mx * my
    a1, a2 = 2.0 * mx * my + c1, 2.0 * sxy + c2
    b1, b2 = mx * mx + my * my + c1, sxx + syy + c2
    ssim_map = a1 * a2 / (b1 * b2)
    scale = float(upstream) / ssim_map.size
    # partial derivatives of the map with respect to the means (central moments held fixed) and the central moments
    d_mx = 2.0 * my * a2 / (b1 * b2) - 2.0 * mx * ssim_map / b1
    d_my = 2.0 * mx * a2 / (b1 * b2) - 2.0 * my * ssim_map / b1
    d_s = -ssim_map / b2             # with respect to sxx and to syy
    d_sxy = 2.0 * a1 / (b1 * b2)
    adj = lambda m: blur_adjoint(m * scale, g, padding)
    dimage = adj(d_mx - 2.0 * mx * d_s - my * d_sxy) + 2.0 * x * adj(d_s) + y * adj(d_sxy)
    dtarget = adj(d_my - 2.0 * my * d_s - mx * d_sxy) + 2.0 * y * adj(d_s) + x * adj(d_sxy)
    return {"value": float(ssim_map.mean()), "map": ssim_map, "dimage": dimage, "dtarget": dtarget}


# ---- the seeded input families of the GPU tests (float32 values, handed to both sides) -------------------------

def noise_pair(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.random(shape, dtype=np.float32), rng.random(shape, dtype=np.float32)


def noisy_copy(shape, seed, amplitude=0.05):
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=np.float32)
    b = np.clip(a + amplitude * rng.standard_normal(shape).astype(np.float32), 0.0, 1.0).astype(np.float32)
    return a, b


def shaded_discs(shape, seed):
    """Two smoothly shaded discs on a zero background, shifted against each other: the render-like case, with flat
    regions where sxx is a difference of nearly equal numbers."""
    B, H, W, C = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = []
    for shift in (0.0, 1.7):
        img = np.zeros(shape, dtype=np.float64)
        for b in range(B):
            cy, cx = 0.5 * H + rng.uniform(-1, 1), 0.5 * W + rng.uniform(-1, 1)
            radius = 0.35 * max(min(H, W), 4)
            d2 = ((yy - cy - shift) ** 2 + (xx - cx - 0.6 * shift) ** 2) / radius ** 2
            inside = d2 < 1.0
            shade = np.sqrt(np.clip(1.0 - d2, 0.0, 1.0))     # a Lambertian sphere seen head on
            for c in range(C):
                img[b, :, :, c] = np.where(inside, (0.35 + 0.15 * c) * (0.3 + 0.7 * shade), 0.0)
            if C == 4:
                img[b, :, :, 3] = inside
        out.append(img.astype(np.float32))
        rng = np.random.default_rng(seed)   # the same centres for the second image: only the shift differs
    return out[0], out[1]


def eager_float32_ssim(image, target, window_size=11, sigma=1.5, padding="same", k1=0.01, k2=0.03, data_range=1.0):
    """The loss as a user would spell it in eager float32 torch (grouped conv2d, blur(x^2) - mu^2), on the tensors'
    device: the comparison of tools/ssim_bench.py and the yardstick of the identical-images test."""
    import torch
    import torch.nn.functional as F
    B, H, W, C = image.shape
    g = torch.from_numpy(window(window_size, sigma).astype(np.float32)).to(image.device)
    kernel = (g[:, None] * g[None, :]).expand(C, 1, window_size, window_size).contiguous()
    pad = window_size // 2 if padding == "same" else 0
    conv = lambda t: F.conv2d(t, kernel, padding=pad, groups=C)
    x, y = image.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    return (((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))).mean()
