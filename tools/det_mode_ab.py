"""Deterministic mode, one native library against another: bit for bit, and (--time) step for step.

    python tools/det_mode_ab.py --lib OLD.so --lib NEW.so [--time] [--out DIR]

Under set_deterministic(True) every gradient is reproducible, so two builds of the library with the same C ABI
can be compared exactly.  Each library gets a fresh child process (MR_NATIVE_LIB_PATH) that runs every
deterministic backward once on seeded inputs and writes the gradients to DIR/<n>.npz; the parent -- which never
touches the GPU -- compares the uint32 views with numpy.array_equal and prints one JSON line.  Exit status 1 if
any array differs.

--time: each child also times, with device events around 200 steps after 10 of warm-up, the diffuse deterministic
step at BASELINE configs[2]'s shape (5k triangles, 1024^2, batch 32; with the L1 spelling -- sign codes -- and
with a dense loss, the one that reads the upstream image for its largest element) and the SoftRas deterministic
step at 512^2, batch 16; and the libraries are run alternately, twice each (old, new, old, new).

Shapes of the comparison: a 50-subdivision sphere at 2 x 320x240 for the per-triangle passes (thousands of
merge-table flushes per image), SoftRas at 64x64 over 288 triangles, a 32x16 RGB texture under a 64x64 UV image.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gradients():
    """{name: numpy array} of every deterministic backward, run once."""
    import torch
    from pytorch_mesh_renderer_amd import _native, mesh_renderer, soft_mesh_renderer
    from pytorch_mesh_renderer_amd.common import synthetic
    from pytorch_mesh_renderer_amd.mesh_renderer.rasterize import rasterize_clip_space
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(2024)
    out = {}
    W, H = 320, 240
    job = synthetic.sphere_job(2, W, H, 50)
    tris = job["triangles"].to(dev)
    clip = job["clip"].to(dev)
    V = job["vertices"].shape[1]

    ids, bary, z = _native.rasterize_forward(clip, tris, W, H)
    dbary = (torch.randn(2, H, W, 3, generator=gen) / (W * H)).to(dev)
    out["raster.dclip"] = _native.rasterize_backward(dbary, clip, tris, ids, bary)

    base = {"vertices": job["vertices"], "normals": job["normals"], "diffuse": torch.rand(2, V, 3, generator=gen),
            "specular": torch.rand(2, V, 3, generator=gen), "shininess": 0.3 + torch.rand(2, V, generator=gen)}
    target = torch.rand(2, H, W, 4, generator=gen).to(dev)
    weights = (torch.randn(2, H, W, 4, generator=gen) / (W * H)).to(dev)
    for shading in ("diffuse", "specular"):
        names = sorted(base) if shading == "specular" else ["diffuse", "normals", "vertices"]
        for loss in ("dense", "l1"):
            leaves = {k: base[k].clone().to(dev).requires_grad_(True) for k in names}
            extra = {}
            if shading == "specular":
                extra = dict(specular_colors=leaves["specular"], shininess_coefficients=leaves["shininess"])
            img = mesh_renderer.render(leaves["vertices"], tris, leaves["normals"], leaves["diffuse"], job["eyes"],
                                       torch.zeros(2, 3), torch.tensor([0.0, 1.0, 0.0]), job["light_positions"].to(dev),
                                       job["light_intensities"].to(dev), W, H, **extra)
            ((img * weights).sum() if loss == "dense" else torch.mean(torch.abs(img - target)) * 20.0).backward()
            for k in names:
                out["%s.%s.d_%s" % (shading, loss, k)] = leaves[k].grad

    c = clip.clone().requires_grad_(True)
    a = torch.rand(2, V, 7, generator=gen).to(dev).requires_grad_(True)
    w7 = (torch.randn(2, H, W, 7, generator=gen) / (W * H)).to(dev)
    (rasterize_clip_space(c, a, tris, W, H, torch.zeros(7, device=dev)) * w7).sum().backward()
    out["interp.dclip"], out["interp.dattrs"] = c.grad, a.grad

    image = torch.rand(2, H, W, 4, generator=gen).to(dev)
    dout = torch.randn(2, H, W, 4, generator=gen).to(dev)
    opp = mesh_renderer.antialias_topology(tris, V)
    out["antialias.dimage"], out["antialias.dclip"] = _native.antialias_backward(dout, image, ids, bary, z, clip, tris, opp)

    soft = synthetic.sphere_job(2, 64, 64, 12)
    leaves = {k: soft[k].clone().to(dev).requires_grad_(True) for k in ("vertices", "diffuse", "light_positions")}
    img = soft_mesh_renderer.render(leaves["vertices"], soft["triangles"].to(dev), leaves["diffuse"], soft["eyes"].to(dev),
                                    torch.zeros(2, 3, device=dev), torch.tensor([0.0, 1.0, 0.0], device=dev),
                                    leaves["light_positions"], torch.ones(2, 1, device=dev), 64, 64)
    (img * (torch.rand(2, 64, 64, 4, generator=gen) / (64 * 64)).to(dev)).sum().backward()
    for k, v in leaves.items():
        out["soft.d_%s" % k] = v.grad

    tex = (torch.rand(16, 32, 3, generator=gen) * 4.0 - 2.0).to(dev)
    uv = (torch.rand(2, 64, 64, 2, generator=gen) * 3.0 - 1.0).to(dev)
    dtex_out = torch.randn(2, 64, 64, 3, generator=gen).to(dev)
    out["texture.dtex"], out["texture.duv"] = _native.texture_backward(dtex_out, tex, uv, None, "wrap")
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def timings(steps=200, warmup=10):
    """{name: ms per step}, device events around `steps` steps."""
    import torch
    from pytorch_mesh_renderer_amd import mesh_renderer, soft_mesh_renderer
    from pytorch_mesh_renderer_amd.common import synthetic
    dev = torch.device("cuda:0")

    def timed(step):
        for _ in range(warmup):
            step()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        for _ in range(steps):
            step()
        end.record()
        torch.cuda.synchronize()
        return round(begin.elapsed_time(end) / steps, 4)

    out = {}
    B, S = 32, 1024
    job = synthetic.sphere_job(B, S, S, 50)
    v = job["vertices"].to(dev).requires_grad_(True)
    args = (job["triangles"].to(dev), job["normals"].to(dev), job["diffuse"].to(dev), job["eyes"], torch.zeros(B, 3),
            torch.tensor([0.0, 1.0, 0.0]), job["light_positions"].to(dev), job["light_intensities"].to(dev), S, S)
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand(B, S, S, 4, generator=gen, device=dev)
    weights = torch.randn(B, S, S, 4, generator=gen, device=dev) / (S * S)

    def diffuse(dense):
        def step():
            v.grad = None
            img = mesh_renderer.render(v, *args)
            ((img * weights).sum() if dense else torch.mean(torch.abs(img - target))).backward()
        return step
    out["diffuse_l1_ms"] = timed(diffuse(False))
    out["diffuse_dense_ms"] = timed(diffuse(True))
    del target, weights, v, args
    torch.cuda.empty_cache()

    B, S = 16, 512
    job = synthetic.sphere_job(B, S, S, 50)
    v5 = job["vertices"].to(dev).requires_grad_(True)
    args5 = (job["triangles"].to(dev), job["diffuse"].to(dev), job["eyes"], torch.zeros(B, 3), torch.tensor([0.0, 1.0, 0.0]),
             job["light_positions"].to(dev), torch.ones(B, 1, device=dev), S, S)

    def soft():
        v5.grad = None
        soft_mesh_renderer.render(v5, *args5).mean().backward()
    out["soft_ms"] = timed(soft)
    return out


def child(path, time_too):
    import numpy as np
    from pytorch_mesh_renderer_amd import _native
    _native.set_deterministic(True)
    np.savez(path, **gradients())
    if time_too:
        print(json.dumps(timings()), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", action="append", default=[], help="native library (give it twice: old, new)")
    ap.add_argument("--time", action="store_true", help="also time the deterministic steps, alternating, twice each")
    ap.add_argument("--out", default="det_mode_ab_out", help="directory for the .npz files")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.time)
    if len(args.lib) != 2:
        ap.error("give --lib twice")
    import numpy as np
    os.makedirs(args.out, exist_ok=True)
    runs = []
    for i, lib in enumerate(args.lib * (2 if args.time else 1)):
        path = os.path.join(args.out, "%d.npz" % i)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", path] + (["--time"] if args.time else [])
        proc = subprocess.run(cmd, env=dict(os.environ, MR_NATIVE_LIB_PATH=os.path.abspath(lib)), stdout=subprocess.PIPE,
                              text=True)
        if proc.returncode != 0:
            raise SystemExit("the run with %s failed (exit status %d)" % (lib, proc.returncode))
        runs.append({"lib": lib, "npz": path, "ms": json.loads(proc.stdout.strip().splitlines()[-1]) if args.time else None})
    first = np.load(runs[0]["npz"])
    different = []
    for other in runs[1:]:
        data = np.load(other["npz"])
        assert sorted(data.files) == sorted(first.files)
        for name in first.files:
            same = first[name].shape == data[name].shape and np.array_equal(
                np.ascontiguousarray(first[name]).view(np.uint32), np.ascontiguousarray(data[name]).view(np.uint32))
            if not same:
                different.append(name)
    result = {"arrays": sorted(first.files), "different": sorted(set(different)), "all_equal": not different}
    if args.time:
        result["ms_per_step"] = [{"lib": r["lib"], **r["ms"]} for r in runs]
    print(json.dumps(result))
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
