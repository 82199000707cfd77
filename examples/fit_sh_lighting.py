"""Recover a spherical-harmonics environment light from images of a sphere.

Renders the K = 50 sphere from four cameras around it under known second-order SH irradiance coefficients, then
recovers one shared [9, 3] set of coefficients from zeros by gradient descent through render_sh().  The image is
linear in the coefficients, so the loss is a well-conditioned quadratic.

    python examples/fit_sh_lighting.py --out /tmp/frames [--steps 300] [--size 128]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from PIL import Image

from pytorch_mesh_renderer_amd import mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

# the coefficients to recover: a warm key light from above and the front right, a cool fill from below
TRUE_SH = [[0.90, 0.85, 0.80], [0.30, 0.25, 0.15], [0.20, 0.22, 0.25], [0.15, 0.10, 0.05], [0.05, 0.04, 0.00],
           [0.08, 0.05, 0.02], [-0.10, -0.08, -0.05], [0.04, 0.02, 0.06], [0.06, 0.03, -0.04]]
# four cameras on the corners of a tetrahedron around the sphere: every normal is seen by at least one of them
EYES = [[1.0, 1.0, 1.0], [-1.0, -1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, -1.0, -1.0]]


def fit(steps=300, size=128, lr=0.05, device="cuda:0", out=None):
    """Adam on the coefficients from zeros; returns the first and last loss and the largest coefficient error."""
    device = torch.device(device)
    vertices, triangles, normals = shapes.sphere(1.0, 50)
    B = len(EYES)
    vertices = vertices.unsqueeze(0).repeat(B, 1, 1).to(device)
    normals = normals.unsqueeze(0).repeat(B, 1, 1).to(device)
    triangles = triangles.to(device)
    diffuse = torch.full_like(vertices, 0.8)
    eyes = torch.tensor(EYES, device=device) * (3.0 / 3.0 ** 0.5)
    center = torch.zeros(B, 3, device=device)
    up = torch.tensor([[0.0, 1.0, 0.0]], device=device).repeat(B, 1)
    true_sh = torch.tensor(TRUE_SH, device=device)

    def image(sh):
        return mesh_renderer.render_sh(vertices, triangles, normals, diffuse, sh, eyes, center, up, size, size)

    with torch.no_grad():
        target = image(true_sh)
    sh = torch.zeros(9, 3, device=device, requires_grad=True)
    optimizer = torch.optim.Adam([sh], lr=lr)
    schedule = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, steps)
    losses = []
    for step in range(steps):
        optimizer.zero_grad()
        loss = torch.mean((image(sh) - target) ** 2)
        loss.backward()
        optimizer.step()
        schedule.step()
        losses.append(float(loss.detach()))
        if out is not None and step % 20 == 0:
            save(image(sh.detach()), os.path.join(out, "frame_%03d.png" % step))
    with torch.no_grad():
        final = float(torch.mean((image(sh) - target) ** 2))
    if out is not None:
        save(target, os.path.join(out, "target.png"))
        save(image(sh.detach()), os.path.join(out, "fitted.png"))
    return {"initial_loss": losses[0], "final_loss": final,
            "coefficient_error": float((sh.detach() - true_sh).abs().max()), "sh": sh.detach().cpu().tolist()}


def save(images, path):
    """The batch side by side as one 8-bit RGB frame."""
    rgb = torch.cat(list(images[..., :3].detach().clamp(0, 1)), dim=1)
    Image.fromarray((rgb * 255).round().to(torch.uint8).cpu().numpy()).save(path)


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--out", default=None)
    parser.add_argument("--steps", type=int, default=300)
    parser.add_argument("--size", type=int, default=128)
    args = parser.parse_args()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    result = fit(steps=args.steps, size=args.size, out=args.out)
    print("loss %.3g -> %.3g, largest coefficient error %.2e" % (
        result["initial_loss"], result["final_loss"], result["coefficient_error"]))


if __name__ == "__main__":
    main()
