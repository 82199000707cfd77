"""Recover an RGB texture from images of a textured sphere with the photometric loss (L1 mixed with SSIM).

fit_texture.py's job -- its sphere, six cameras, true texture and seen-texel measure, imported from there -- scored
by losses.photometric_loss, (1 - w) mean|image - target| + w (1 - SSIM), instead of the mean squared error: the
structural term weighs the checker's edges, which a per-pixel loss only sees as a few pixels of error.

    python examples/fit_texture_photometric.py --out /tmp/frames [--steps 300] [--size 128] [--ssim-weight 0.2]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from fit_texture import EYES, TEXTURE_H, TEXTURE_W, UPS, save, save_texture, true_texture
from pytorch_mesh_renderer_amd import mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer.losses import photometric_loss


def fit(steps=300, size=128, lr=0.05, ssim_weight=0.2, device="cuda:0", out=None):
    """Adam on the texture from grey; returns the first and last photometric loss and the mean texel error, before
    and after, over the texels the views see (a total bilinear weight of at least one pixel)."""
    device = torch.device(device)
    vertices, triangles, _ = shapes.sphere(1.0, 50)
    uvs, uv_triangles = shapes.sphere_uvs(50)
    B = len(EYES)
    vertices = vertices.unsqueeze(0).repeat(B, 1, 1).to(device)
    triangles, uvs, uv_triangles = triangles.to(device), uvs.to(device), uv_triangles.to(device)
    eyes = torch.tensor(EYES, device=device)
    ups = torch.tensor(UPS, device=device)
    center = torch.zeros(B, 3, device=device)
    target_texture = true_texture(device)

    def image(tex):
        return mesh_renderer.render_textured(vertices, triangles, uvs, tex, eyes, center, ups, size, size,
                                             uv_triangles=uv_triangles)

    with torch.no_grad():
        target = image(target_texture)
    probe = torch.zeros_like(target_texture, requires_grad=True)
    image(probe)[..., :3].sum().backward()
    seen = probe.grad[..., 0] >= 1.0

    texture = torch.full((TEXTURE_H, TEXTURE_W, 3), 0.5, device=device, requires_grad=True)
    texel_error = lambda: float((texture.detach() - target_texture).abs().mean(-1)[seen].mean())
    initial_error = texel_error()
    optimizer = torch.optim.Adam([texture], lr=lr)
    schedule = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, steps)
    history = []
    for step in range(steps):
        optimizer.zero_grad()
        loss = photometric_loss(image(texture), target, ssim_weight=ssim_weight)
        loss.backward()
        optimizer.step()
        schedule.step()
        history.append(float(loss.detach()))
        if out is not None and step % 20 == 0:
            save(image(texture.detach()), os.path.join(out, "frame_%03d.png" % step))
    with torch.no_grad():
        final = float(photometric_loss(image(texture), target, ssim_weight=ssim_weight))
    if out is not None:
        save(target, os.path.join(out, "target.png"))
        save(image(texture.detach()), os.path.join(out, "fitted.png"))
        save_texture(texture.detach(), os.path.join(out, "texture_fitted.png"))
        save_texture(target_texture, os.path.join(out, "texture_target.png"))
    return {"initial_loss": history[0], "final_loss": final, "initial_texel_error": initial_error,
            "final_texel_error": texel_error(), "seen_texels": int(seen.sum())}


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--out", default=None)
    parser.add_argument("--steps", type=int, default=300)
    parser.add_argument("--size", type=int, default=128)
    parser.add_argument("--ssim-weight", type=float, default=0.2)
    args = parser.parse_args()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    result = fit(steps=args.steps, size=args.size, ssim_weight=args.ssim_weight, out=args.out)
    print("photometric loss %.3g -> %.3g, mean texel error %.3g -> %.3g over %d seen texels" % (
        result["initial_loss"], result["final_loss"], result["initial_texel_error"], result["final_texel_error"],
        result["seen_texels"]))


if __name__ == "__main__":
    main()
