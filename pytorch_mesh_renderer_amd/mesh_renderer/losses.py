"""Image losses used with the renderer.

The reference has no loss module; its tests and examples spell the loss out as
`torch.mean(torch.abs(render - target))` (src/mesh_renderer/mesh_renderer_test.py:250,
src/examples/example5.py:70-92).  In eager torch that is five passes over the image; this is
the same quantity as one HIP pass forward (which also packs sign(image - target), 2 bits per
element) and one backward that reads only those signs.

ssim / photometric_loss: the structural-similarity loss (Wang et al. 2004) and its usual mix with L1, one HIP
stencil pass forward and one backward (csrc/ssim.hip) instead of five grouped convolutions and their autograd chain.
"""
import ctypes

import torch

from .. import _native


class _MeanAbsError(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, target):
        need_grad = any(ctx.needs_input_grad)
        loss, signs = _native.l1_loss_forward(image.detach(), target.detach(), want_signs=need_grad)
        if need_grad:
            ctx.save_for_backward(signs)  # 1 byte per pixel instead of both images
        ctx.shape = image.shape
        return loss

    @staticmethod
    def backward(ctx, grad):
        (signs,) = ctx.saved_tensors
        da = _native.l1_loss_backward(signs, ctx.shape, grad.to(torch.float32).reshape(1))
        return (da if ctx.needs_input_grad[0] else None), (-da if ctx.needs_input_grad[1] else None)


import os

USE_FUSED_RENDER_LOSS = os.environ.get("MR_FUSED_RENDER_LOSS", "1") != "0"   # False: always the generic op (dense gradient image)


def remember_target(target):
    """Opt-in for a FIXED loss target (an optimisation loop compares every step's render with the same image): finds
    which 64 x 64 blocks of `target` are all zeros, once, and keeps that map on the tensor; see l1_loss, TARGET.

    The renderer also learns of the target (one weak reference to the most recently remembered target per device and
    shape): a differentiable render() of that shape on the fused diffuse path then compares each pixel with the target
    while it still holds it in registers, and l1_loss(image, target) -- or torch.mean(torch.abs(image - target)) --
    picks the loss and its sign codes up from there: the loss kernel and its re-read of the image (16 B/px) do not
    run.  The price: a render() of the same shape made for ANOTHER purpose while the target is remembered pays one
    extra read of the target (16 B/px); forget_target(target) ends that.  Calling remember_target again on the same
    tensor (after target.copy_(new)) refreshes the map in place, so a captured step (capture_step) follows it."""
    from .rasterize_triangles_ext import remember_target_map
    remember_target_map(target)
    return target


def forget_target(target):
    """Drops remember_target's map and the renderer's reference to the target."""
    from .rasterize_triangles_ext import forget_target_map
    forget_target_map(target)


def l1_loss(image, target):
    """mean(|image - target|) over every element; same value and gradients as
    torch.mean(torch.abs(image - target)) (sign(0) = 0) -- which, written on render()'s own output, arrives here by
    itself (mesh_renderer/rendered_image.py).

    When `image` is the direct output of render()'s fused diffuse path, the backward skips the
    dense gradient image: the loss's sign codes go straight into the shading backward
    (rasterize_triangles_ext.FusedPhongL1Loss; FusedSpecularL1Loss for the specular path, round 5).  Whether something observes d loss / d image -- image.retain_grad(),
    a hook on the image, torch.autograd.grad(loss, image) -- is decided when the BACKWARD runs (round 5; until then it
    was decided here, and a hook registered after this call never fired): the node then behaves like the generic op.
    (loss.backward(inputs=[image]) is seen too: the engine retain_grad()s what it is given.)
    USE_FUSED_RENDER_LOSS = False takes the generic op always.

    TARGET: on that route the 64 x 64 blocks that are all zeros in BOTH images are not read, if the caller has
    named the target with remember_target(target): the renderer knows its own empty blocks, the target's map is made by
    that call and used while the tensor's data pointer, shape and autograd version counter stay what they were (any
    in-place torch operation on the target moves the counter: the loss then reads every block until the next
    remember_target).  MR_EMPTY_REGIONS=0 switches the maps off."""
    if image.shape != target.shape:
        raise ValueError("image and target must have the same shape")
    if image.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError("l1_loss expects float32 tensors")
    if USE_FUSED_RENDER_LOSS and torch.is_grad_enabled() and image.requires_grad:
        from .rasterize_triangles_ext import FusedPhongL1Loss, FusedSpecularL1Loss, take_fused_render
        record = take_fused_render(image)
        if record is not None and record["kind"] == "specular":
            return FusedSpecularL1Loss.apply(image, target, *record["inputs"], record["saved"],
                                             record["has_ambient"], record["has_transforms"])
        if record is not None:
            return FusedPhongL1Loss.apply(image, target, *record["inputs"], record["saved"],
                                          record.get("prepared_state"), record.get("empty_regions"),
                                          record.get("l1_in_forward"))
    return _MeanAbsError.apply(image, target)


class _MeanSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, target, window_size, sigma, padding, c1, c2):
        grads = (_native.SSIM_GRAD_IMAGE if ctx.needs_input_grad[0] else 0) | \
                (_native.SSIM_GRAD_TARGET if ctx.needs_input_grad[1] else 0)
        image, target = image.detach(), target.detach()
        value, _, saved = _native.ssim_forward(image, target, window_size, sigma, padding, c1, c2, grads=grads)
        if grads:
            ctx.save_for_backward(image, target, saved)
        ctx.config = (window_size, sigma, padding, grads)
        return value

    @staticmethod
    def backward(ctx, grad):
        image, target, saved = ctx.saved_tensors
        window_size, sigma, padding, grads = ctx.config
        da, db = _native.ssim_backward(image, target, saved, grad.to(torch.float32).reshape(1), window_size, sigma,
                                       padding, grads, want_image=ctx.needs_input_grad[0],
                                       want_target=ctx.needs_input_grad[1])
        return da, db, None, None, None, None, None


def _ssim_arguments(image, target, window_size=11, sigma=1.5, padding="same", k1=0.01, k2=0.03, data_range=1.0):
    """Checks everything ssim() takes, before anything is launched -> (window_size, sigma, padding, C1, C2)."""
    _native._chk_ssim(image, target, window_size, sigma, padding)
    for name, v in (("k1", k1), ("k2", k2), ("data_range", data_range)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0.0 < float(v) < float("inf")):
            # (C1 = 0 or C2 = 0 makes the map 0 / 0 wherever both images are flat, e.g. a render's empty background)
            raise ValueError("%s must be a positive finite number, got %r" % (name, v))
    c1, c2 = (ctypes.c_float((float(k) * float(data_range)) ** 2).value for k in (k1, k2))   # as the kernels get them
    if not (0.0 < c1 < float("inf") and 0.0 < c2 < float("inf")):
        raise ValueError("(k1 data_range)^2 and (k2 data_range)^2 must be positive float32 numbers, got %r, %r" % (c1, c2))
    return window_size, float(sigma), padding, c1, c2


def ssim(image, target, window_size=11, sigma=1.5, padding="same", k1=0.01, k2=0.03, data_range=1.0):
    """Mean structural similarity of two [B, H, W, C] float32 images (1 <= C <= 4, channels independent) as a 0-D
    tensor, differentiable in both.  Per channel and pixel, with G the window_size x window_size Gaussian of `sigma`
    (normalised to sum 1):

        mx = G*x   my = G*y   sxx = G*(x x) - mx^2   syy = G*(y y) - my^2   sxy = G*(x y) - mx my
        ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sxx + syy + C2)),   C1 = (k1 data_range)^2, C2 likewise

    padding="same": taps outside the image contribute zero (conv2d(padding=window_size // 2)) and the map is H x W;
    "valid": only windows wholly inside, H, W >= window_size.  The value is the plain mean of the map.  k1, k2 and
    data_range must be positive.  A gradient that is not required is not computed, and under no_grad nothing is
    saved for one; both gradients are gathers without atomics and bit-reproducible."""
    arguments = _ssim_arguments(image, target, window_size, sigma, padding, k1, k2, data_range)
    if not torch.is_grad_enabled():   # (needs_input_grad does not look at the grad mode)
        return _native.ssim_forward(image.detach(), target.detach(), *arguments, grads=0)[0]
    return _MeanSSIM.apply(image.contiguous(), target.contiguous(), *arguments)


def photometric_loss(image, target, ssim_weight=0.2, **ssim_arguments):
    """(1 - w) l1_loss(image, target) + w (1 - ssim(image, target, **ssim_arguments)), w = ssim_weight in [0, 1].

    The L1 part is l1_loss itself: on render()'s own output it keeps the fused route (sign codes straight into the
    shading backward), and the SSIM part's dense gradient reaches the renderer through the image's node; the two
    contributions add up there.  Every argument is checked whatever the weight; a part whose weight is zero is not
    computed."""
    if isinstance(ssim_weight, bool) or not isinstance(ssim_weight, (int, float)) or not 0.0 <= ssim_weight <= 1.0:
        raise ValueError("ssim_weight must be a number in [0, 1], got %r" % (ssim_weight,))
    _ssim_arguments(image, target, **ssim_arguments)   # (an unknown keyword is a TypeError here, at any weight)
    w = float(ssim_weight)
    if w == 0.0:
        return l1_loss(image, target)
    if w == 1.0:
        return 1.0 - ssim(image, target, **ssim_arguments)
    return (1.0 - w) * l1_loss(image, target) + w * (1.0 - ssim(image, target, **ssim_arguments))
