"""An independent float64 restatement of bilinear texture sampling ("Texture mapping").

Only the tap decision is binary32, as specified: x = fl(fl(u * Wt) - 0.5f), y likewise; everything after it is
float64.  Works on CPU or device tensors.
"""
import torch

LIMIT = float(2 ** 24)


def _coords(uv, Ht, Wt):
    uv32 = uv.to(torch.float32)
    x = uv32[..., 0] * torch.tensor(float(Wt), dtype=torch.float32)      # one rounding ...
    x = x - torch.tensor(0.5, dtype=torch.float32)                       # ... and the second
    y = uv32[..., 1] * torch.tensor(float(Ht), dtype=torch.float32)
    y = y - torch.tensor(0.5, dtype=torch.float32)
    return x, y


def _index(i, n, boundary):
    return torch.remainder(i, n) if boundary == "wrap" else i.clamp(0, n - 1)


def taps(uv, Ht, Wt, mask=None, boundary="wrap"):
    """-> (valid [B,H,W] bool, fx, fy float64, and the four taps' (row, column) index pairs, each [B,H,W] long,
    in the order (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1))."""
    x, y = _coords(uv, Ht, Wt)
    valid = torch.isfinite(x) & torch.isfinite(y) & (x.abs() < LIMIT) & (y.abs() < LIMIT)
    if mask is not None:
        valid &= mask > 0.5
    x = torch.where(valid, x, torch.zeros_like(x))
    y = torch.where(valid, y, torch.zeros_like(y))
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = (x - x0).double(), (y - y0).double()
    ix, iy = x0.long(), y0.long()
    xa, xb = _index(ix, Wt, boundary), _index(ix + 1, Wt, boundary)
    ya, yb = _index(iy, Ht, boundary), _index(iy + 1, Ht, boundary)
    return valid, fx, fy, [(ya, xa), (ya, xb), (yb, xa), (yb, xb)]


def _weights(fx, fy):
    return [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]


def _batched(tex, B):
    return tex.double() if tex.dim() == 4 else tex.double().unsqueeze(0).expand(B, *tex.shape)


def sample(tex, uv, mask=None, boundary="wrap", dout=None):
    """tex [Ht,Wt,C] or [B,Ht,Wt,C], uv [B,H,W,2] -> value [B,H,W,C] float64.  With dout [B,H,W,C] also the
    gradients: -> (value, dtex (tex's shape), duv [B,H,W,2], abs_sum (tex's shape: the sum of |contribution| per
    texel and channel, the scale of dtex's rounding))."""
    B = uv.shape[0]
    Ht, Wt, C = tex.shape[-3:]
    t = _batched(tex, B)
    valid, fx, fy, tp = taps(uv, Ht, Wt, mask, boundary)
    bi = torch.arange(B, device=uv.device).view(B, 1, 1).expand(valid.shape)
    w = _weights(fx, fy)
    vals = [t[bi, r, c] for r, c in tp]                                  # 4 x [B,H,W,C]
    value = sum(wk.unsqueeze(3) * vk for wk, vk in zip(w, vals))
    value = torch.where(valid.unsqueeze(3), value, torch.zeros_like(value))
    if dout is None:
        return value
    g = torch.where(valid.unsqueeze(3), dout.double(), torch.zeros_like(value))
    t00, t01, t10, t11 = vals
    du = Wt * (g * ((1 - fy).unsqueeze(3) * (t01 - t00) + fy.unsqueeze(3) * (t11 - t10))).sum(3)
    dv = Ht * (g * ((1 - fx).unsqueeze(3) * (t10 - t00) + fx.unsqueeze(3) * (t11 - t01))).sum(3)
    duv = torch.stack([du, dv], 3)
    dtex = torch.zeros(B * Ht * Wt, C, dtype=torch.float64, device=uv.device)
    abs_sum = torch.zeros_like(dtex)
    for wk, (r, c) in zip(w, tp):
        flat = ((bi * Ht + r) * Wt + c).reshape(-1)
        contrib = (wk.unsqueeze(3) * g).reshape(-1, C)
        dtex.index_add_(0, flat, contrib)
        abs_sum.index_add_(0, flat, contrib.abs())
    dtex, abs_sum = dtex.view(B, Ht, Wt, C), abs_sum.view(B, Ht, Wt, C)
    if tex.dim() == 3:
        dtex, abs_sum = dtex.sum(0), abs_sum.sum(0)
    return value, dtex, duv, abs_sum
