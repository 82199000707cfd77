"""Autograd boundary of the HIP rasterizer.

Drop-in for src/mesh_renderer/rasterize_triangles_ext.py:6-63: same class name,
same forward / backward signatures and return tuples.  The reference's class
rasterizes ONE image per call; this one also accepts a batch ([B,V,4]) so that
rasterize_clip_space does not need a Python loop over images
(src/mesh_renderer/rasterize.py:112-121) -- on MI355X the batch is the grid.
"""
import contextlib
import os
import threading
import weakref

import torch

from .. import _native


class BarycentricRasterizer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, clip_space_vertices, triangles, image_width, image_height):
        """clip_space_vertices [V,4] or [B,V,4] f32, triangles [T,3] i32 ->
        (px_triangle_ids [.., H, W] i32, px_barycentric_coords [.., H, W, 3] f32,
         z_buffer [.., H, W] f32); ids are 0, barycentrics 0 and z 1.0 where no
        triangle was drawn; row 0 is the bottom scanline."""
        unbatched = clip_space_vertices.dim() == 2
        clip = clip_space_vertices.detach()
        if unbatched:
            clip = clip.unsqueeze(0)
        if clip.dtype != torch.float32:
            raise RuntimeError("clip_space_vertices must be float32")
        if triangles.dtype != torch.int32:
            raise RuntimeError("triangles must be int32")
        ids, bary, z = _native.rasterize_forward(clip, triangles, int(image_width), int(image_height))
        ctx.save_for_backward(clip, triangles, ids, bary)
        ctx.unbatched = unbatched
        ctx.mark_non_differentiable(ids)
        if unbatched:
            return ids[0], bary[0], z[0]
        return ids, bary, z

    @staticmethod
    def backward(ctx, _, df_dbarycentric_coords, __):
        """Gradient w.r.t. clip-space vertices only; triangles get zeros, sizes None
        and the gradient of z is ignored, as in the reference (:46-63)."""
        clip, triangles, ids, bary = ctx.saved_tensors
        dbary = df_dbarycentric_coords
        if ctx.unbatched:
            dbary = dbary.unsqueeze(0)
        dclip = _native.rasterize_backward(dbary.contiguous(), clip, triangles, ids, bary)
        if ctx.unbatched:
            dclip = dclip[0]
        return dclip, torch.zeros_like(triangles), None, None


class AttributeInterpolator(torch.autograd.Function):
    """Deferred attribute interpolation + alpha / background blend as one HIP op.

    Fuses the gather / multiply / sum / clamp / blend block of
    src/mesh_renderer/rasterize.py:118-150 and its autograd backward."""

    @staticmethod
    def forward(ctx, ids, bary, attributes, triangles, background):
        out = _native.interpolate_forward(ids, bary.detach(), attributes.detach(), triangles,
                                          background.detach())
        ctx.save_for_backward(ids, bary.detach(), attributes.detach(), triangles, background.detach())
        return out

    @staticmethod
    def backward(ctx, dout):
        ids, bary, attributes, triangles, background = ctx.saved_tensors
        dattrs, dbary = _native.interpolate_backward(dout.contiguous(), ids, bary, attributes,
                                                     triangles, background)
        dbackground = None
        if ctx.needs_input_grad[4]:
            # d/d background = sum over pixels of (1 - alpha) * dout  (rasterize.py:149-150)
            alpha = torch.clamp(2.0 * bary.sum(-1, keepdim=True), 0.0, 1.0)
            dbackground = ((1.0 - alpha) * dout).sum(dim=(0, 1, 2))
        return None, dbary, dattrs, None, dbackground


# False (or MR_FUSED_INTERPOLATION=0 in the environment at import): k_raster, then k_interp_forward_rec over the G-buffer
FUSED_INTERPOLATION_EPILOGUE = os.environ.get("MR_FUSED_INTERPOLATION", "1") != "0"


class FusedAttributeRasterizer(torch.autograd.Function):
    """rasterize_clip_space() as ONE differentiable op for up to 16 attributes: G-buffer
    rasterization + attribute interpolation forward, and a single pass over the G-buffer backward
    that yields dL/dattributes and dL/dclip together (src/mesh_renderer/rasterize.py:66-152 and
    rasterize_triangles.cpp:131-273 behind it)."""

    @staticmethod
    def forward(ctx, clip, attributes, triangles, background, image_width, image_height):
        clip_d = clip.detach().contiguous()
        attrs_d, bg_d = attributes.detach().contiguous(), background.detach().contiguous()
        if FUSED_INTERPOLATION_EPILOGUE:   # round 4: one pass over the pixels (the interpolation is k_raster's epilogue)
            ids, bary, out, records = _native.rasterize_interpolate_forward(clip_d, attrs_d, triangles, bg_d,
                                                                            int(image_width), int(image_height))
        else:
            ids, bary, _ = _native.rasterize_forward(clip_d, triangles, int(image_width), int(image_height))
            out, records = _native.interpolate_forward_records(ids, bary, attrs_d, triangles, bg_d)
        offsets, entries = _native.vertex_adjacency(triangles, clip_d.shape[1])   # cached per mesh
        ctx.save_for_backward(clip_d, ids, bary, attrs_d, triangles, bg_d, offsets, entries, records)
        return out

    @staticmethod
    def backward(ctx, dout):
        clip, ids, bary, attributes, triangles, background, offsets, entries, records = ctx.saved_tensors
        dout = dout.contiguous()
        dattrs, dclip = _native.interpolate_raster_backward(dout, ids, bary, clip, attributes, triangles,
                                                            background, (offsets, entries),
                                                            corner_records=records,
                                                            normalised_gbuffer=True)   # forward() above wrote ids / bary
        dbackground = None
        if ctx.needs_input_grad[3]:
            # d/d background = sum over pixels of (1 - alpha) * dout  (rasterize.py:149-150)
            alpha = torch.clamp(2.0 * bary.sum(-1, keepdim=True), 0.0, 1.0)
            dbackground = ((1.0 - alpha) * dout).sum(dim=(0, 1, 2))
        return dclip, dattrs, None, dbackground, None, None


# Switches of FusedPhongRenderer's forward.  They are scoped to a `with` block of the calling thread
# (round 2 flipped module globals from the benchmark: whichever thread set them last won):
#   shading_epilogue(False)  k_raster, then k_shade_forward over the G-buffer, instead of one pass over
#                            the pixels (mr_render_forward: the shading is the epilogue of the
#                            rasterizer's tile walk).  For measurements and the parity tests.
#   emit_uint8_frames(True)  the one-pass forward also writes the image as 8-bit frames (4 B/px of
#                            stores) and render() attaches them to the image it returns;
#                            mesh_renderer.to_uint8(image) then hands them out instead of converting
#                            the float image in a pass of its own.  For callers that export every frame
#                            (the multi-GPU hand-over of bench.py).
#   loss_in_forward(False)   the one-pass forward does NOT compute mean|image - target| for a remembered target
#                            (losses.remember_target): the loss kernel reads the image back, as it does for any other
#                            target.  For A/B runs and the parity tests.
#   private_gbuffer(False)   the loss-in-forward route keeps the public G-buffer (ids 0 on background, barycentric
#                            plane) even when only the vertices require grad.  On (the default) that route writes no
#                            barycentric plane: the backward's lane kernel rebuilds them (mr_render_forward_l1_private),
#                            and whoever needs the public G-buffer after all -- a second backward over a retained graph,
#                            a dense image gradient -- gets it from one plain rasterizer pass over the saved inputs.
#                            For A/B runs and the parity tests.
# Defaults come from the environment (MR_SHADING_EPILOGUE, MR_EMIT_UINT8_FRAMES, MR_LOSS_IN_FORWARD, MR_PRIVATE_GBUFFER)
# once, at import.
_DEFAULTS = {"shading_epilogue": os.environ.get("MR_SHADING_EPILOGUE", "1") != "0",
             "emit_uint8_frames": os.environ.get("MR_EMIT_UINT8_FRAMES", "0") != "0",
             "loss_in_forward": os.environ.get("MR_LOSS_IN_FORWARD", "1") != "0",
             "private_gbuffer": os.environ.get("MR_PRIVATE_GBUFFER", "1") != "0"}
_scoped = threading.local()


def _switch(name):
    return getattr(_scoped, name, _DEFAULTS[name])


@contextlib.contextmanager
def _scoped_switch(name, value):
    had, before = hasattr(_scoped, name), getattr(_scoped, name, None)
    setattr(_scoped, name, bool(value))
    try:
        yield
    finally:
        if had:
            setattr(_scoped, name, before)
        else:
            delattr(_scoped, name)


def shading_epilogue(on):
    """with shading_epilogue(False): render(...) -- see the comment above."""
    return _scoped_switch("shading_epilogue", on)


def emit_uint8_frames(on):
    """with emit_uint8_frames(True): image = render(...); frames = to_uint8(image)."""
    return _scoped_switch("emit_uint8_frames", on)


def loss_in_forward(on):
    """with loss_in_forward(False): image = render(...) -- see the comment above."""
    return _scoped_switch("loss_in_forward", on)


def private_gbuffer(on):
    """with private_gbuffer(False): image = render(...) -- see the comment above."""
    return _scoped_switch("private_gbuffer", on)


PREPARE_BACKWARD = True   # False: the backward always runs its own setup kernel (A/B, tests)
# False (or MR_EMPTY_REGIONS=0 at import): no empty-block map -- the loss and the backward read every pixel (A/B, tests)
EMPTY_REGIONS = os.environ.get("MR_EMPTY_REGIONS", "1") != "0"


class FusedPhongRenderer(torch.autograd.Function):
    """World-space vertices -> shaded image as ONE differentiable op: clip-space transform,
    G-buffer rasterization, attribute interpolation and diffuse/ambient Phong in four launches
    forward (one pass over the pixels: k_raster with the shading epilogue), one pass over the
    G-buffer backward.  Used by render() when no specular term is requested; covers
    src/common/camera_utils.py:142-170, src/mesh_renderer/rasterize.py:66-152 and
    src/mesh_renderer/render.py:199-228, 287-323, 373-386 and their autograd graph.

    transforms [B,4,4]: the clip-space transforms (perspective . look_at); differentiable -- the
    examples optimise cameras through them -- via one small batched product in the backward."""

    @staticmethod
    def forward(ctx, vertices, transforms, normals, diffuse, triangles, light_positions,
                light_intensities, ambient, image_width, image_height):
        verts, xf = vertices.detach().contiguous(), transforms.detach().contiguous()
        args = [t.detach().contiguous() for t in (normals, diffuse)]
        lp, li = light_positions.detach().contiguous(), light_intensities.detach().contiguous()
        amb = ambient.detach().contiguous() if ambient is not None else None
        frames = None
        epilogue, want_frames = _switch("shading_epilogue"), _switch("emit_uint8_frames")
        # Round 4: when the image will be differentiated to the vertices ONLY (needs_input_grad: the usual
        # optimisation loop), the forward's setup kernel also leaves the folded backward's records and cleared
        # accumulators (`prepared`): the backward then has no setup launch.
        needs = ctx.needs_input_grad
        prepare = bool(epilogue and PREPARE_BACKWARD and needs[0] and not any(needs[i] for i in (1, 2, 3, 5, 6, 7))
                       and not _native.deterministic())
        prepared = None
        empty_regions = None
        # The loss in the forward: the caller has named a fixed target of this image's shape (losses.remember_target) and
        # will differentiate the image -- the usual step is loss(image, target).backward().  The epilogue then reads
        # the target next to the pixel it is about to store and leaves mean|image - target| and its sign codes;
        # FusedPhongL1Loss picks them up if it is handed that very target (and runs the loss kernel for any other).
        l1_target = l1_map = None
        ctx.l1_in_forward = None
        if epilogue and any(needs) and _switch("loss_in_forward"):
            l1_target, l1_map = _remembered_target(verts.device, (verts.shape[0], int(image_height), int(image_width), 4))
        # Both decisions taken -- the loss comes out of this pass and only the vertices require grad -- the G-buffer has one
        # reader, this node's own backward through the sign codes: it is written without its barycentric plane, with -1
        # for background (see private_gbuffer above; one to four lights: the kernel that reads it keeps them in registers).
        private = bool(prepare and l1_target is not None and _switch("private_gbuffer") and lp.shape[1] <= 4)
        if epilogue:
            out = _native.render_forward(
                verts, xf, args[0], args[1], triangles, lp, li, amb, int(image_width), int(image_height),
                want_z=False, want_u8=bool(want_frames), prepare_backward=prepare, want_empty_regions=EMPTY_REGIONS,
                l1_target=l1_target.detach() if l1_target is not None else None,
                l1_target_empty=l1_map if EMPTY_REGIONS else None, private_gbuffer=private)
            if l1_target is not None:
                ctx.l1_in_forward = {"target_key": _target_key(l1_target), "loss": out[-1][0], "signs": out[-1][1]}
                out = out[:-1]
            clip, ids, bary, _, rgba, corner_records = out[:6]
            if private:   # (a placeholder in the saved list; _input_grads never hands it on)
                bary = torch.empty(0, dtype=torch.float32, device=verts.device)
            if want_frames:
                frames = out[6]
            if EMPTY_REGIONS:   # which 64 x 64 blocks of the image are known to be empty (the loss and the backward skip them)
                empty_regions = out[7] if want_frames else out[6]
            if prepare:
                prepared = out[-1]
        else:
            from ..common import camera_utils
            clip = camera_utils.transform_homogeneous(xf, verts).contiguous()
            ids, bary, _ = _native.rasterize_forward(clip, triangles, int(image_width), int(image_height))
            rgba, corner_records = _native.shade_forward(ids, bary, args[0], verts, args[1], triangles, lp,
                                                         li, amb, keep_corner_records=True)
        offsets, entries = _native.vertex_adjacency(triangles, vertices.shape[1])   # cached per mesh
        saved = [clip, ids, bary, args[0], verts, args[1], triangles, lp, li, corner_records,
                 offsets, entries, xf,
                 prepared if prepared is not None else torch.empty(0, dtype=torch.uint8, device=verts.device)]
        if amb is not None:
            saved.append(amb)
        ctx.save_for_backward(*saved)
        ctx.has_ambient = amb is not None
        # the prepared block serves ONE backward call (its accumulator rows are left dirty): a second backward over
        # a retained graph -- through this node or through FusedPhongL1Loss, which shares this dict -- runs the
        # backward's own setup kernel instead
        # "private": ids / bary above are the private G-buffer; "public": the (ids, bary) of the plain rasterizer pass that
        # replaced them, once somebody needed it (_input_grads)
        ctx.prepared_state = {"used": prepared is None, "private": bool(epilogue and private), "public": None}
        ctx.empty_regions = empty_regions
        if frames is not None:
            ctx.mark_non_differentiable(frames)
        # FusedPhongL1Loss on this image hands it NO gradient (it differentiates straight to the inputs above): the
        # node is then called with None and returns at once instead of running a backward over materialised zeros
        ctx.set_materialize_grads(False)
        from .rendered_image import wrap
        return wrap(rgba), frames

    @staticmethod
    def _input_grads(saved, needs_transform_grad, needs_light_grads, upstream, l1_signs=None,
                     needs_normal_grad=True, needs_diffuse_grad=True, prepared_state=None, empty_regions=None):
        """The shading backward on the tensors forward() saved -> gradients in the order of forward()'s
        tensor arguments (vertices, transforms, normals, diffuse, None, lights..., ambient).
        needs_light_grads: some of light_positions / light_intensities / ambient requires grad;
        needs_normal_grad / needs_diffuse_grad: False leaves that gradient (None) and its sums out."""
        (clip, ids, bary, normals, verts, diffuse, triangles, lp, li, corner_records, offsets,
         entries, xf, prepared) = saved[:14]
        amb = saved[14] if len(saved) > 14 else None
        use_prepared = prepared.numel() > 0 and prepared_state is not None and not prepared_state["used"]
        if use_prepared:
            prepared_state["used"] = True
        private = False
        if prepared_state is not None and prepared_state.get("private"):
            # The private G-buffer serves the call it was written for: the first backward, through the sign codes, to the
            # vertices alone, on the lane kernel.  Anything else reads the public one -- the plain rasterizer pass on the
            # saved clip-space vertices, the same kernel and deterministic: the ids and barycentrics the fused forward
            # would have stored -- made once and kept.  (The private block begins with the public one: it still serves.)
            private = (use_prepared and l1_signs is not None and prepared_state["public"] is None
                       and not (needs_transform_grad or needs_light_grads or needs_normal_grad or needs_diffuse_grad)
                       and not _native.deterministic() and _native._shade_backward_kernel != 1)
            if private:
                bary = None
            else:
                if prepared_state["public"] is None:
                    prepared_state["public"] = _native.rasterize_forward(clip, triangles, ids.shape[2], ids.shape[1])[:2]
                ids, bary = prepared_state["public"]
        dclip, dn, dverts, dd, dlp, dli, damb = _native.shade_backward(
            upstream, ids, bary, clip, normals, verts, diffuse, triangles, lp, li, amb,
            corner_records=corner_records, adjacency=(offsets, entries), l1_signs=l1_signs, transforms=xf,
            want_light_grads=needs_light_grads, want_normal_grads=needs_normal_grad,
            want_diffuse_grads=needs_diffuse_grad,
            want_clip_grads=needs_transform_grad,   # d clip on its own only feeds d transforms below
            prepared=prepared if use_prepared else None, empty_regions=empty_regions,
            normalised_gbuffer=True,   # this function's own forward wrote ids / bary
            private_gbuffer=private)
        dxf = None
        if needs_transform_grad:  # d clip[b,v,r] / d xf[b,r,k] = (vertex, 1)[k]
            ones = torch.ones(verts.shape[0], verts.shape[1], 1, dtype=verts.dtype, device=verts.device)
            dxf = torch.matmul(dclip.transpose(1, 2), torch.cat([verts, ones], dim=2))
        return dverts, dxf, dn, dd, None, dlp, dli, damb

    @staticmethod
    def backward(ctx, drgba, _dframes=None):
        if drgba is None:   # (set_materialize_grads(False): nothing upstream depends on the image's values)
            return (None,) * 10
        grads = FusedPhongRenderer._input_grads(ctx.saved_tensors, ctx.needs_input_grad[1],
                                                any(ctx.needs_input_grad[5:8]), drgba.contiguous(),
                                                needs_normal_grad=ctx.needs_input_grad[2],
                                                needs_diffuse_grad=ctx.needs_input_grad[3],
                                                prepared_state=ctx.prepared_state, empty_regions=ctx.empty_regions)
        return grads + (None, None)


# render()'s fused diffuse outputs, by autograd node: what FusedPhongL1Loss needs to differentiate a
# loss on that image straight to the renderer's inputs.  Weak keys: an entry lives as long as its
# node does, and holds only tensors the node holds anyway.
_fused_renders = weakref.WeakKeyDictionary()


def remember_fused_render(node, inputs, image=None, kind="diffuse"):
    _fused_renders[node] = {"saved": tuple(node.saved_tensors), "inputs": inputs, "kind": kind,
                            "has_ambient": getattr(node, "has_ambient", None),
                            "has_transforms": getattr(node, "has_transforms", None),
                            "prepared_state": getattr(node, "prepared_state", None),
                            "empty_regions": getattr(node, "empty_regions", None),
                            # {target_key, loss, signs}: the forward compared the image with the remembered target
                            "l1_in_forward": getattr(node, "l1_in_forward", None),
                            # the empty-block map describes what the renderer WROTE: an in-place edit of the image
                            # (image[..., 3] = 1 under no_grad keeps the grad_fn) bumps this counter and voids it
                            "image_version": image._version if image is not None else None}


def take_fused_render(image):
    """The record of render()'s node behind `image` (None when `image` is not render()'s own output: a tensor derived
    from it has another node).  The record stays with the node: any number of losses may be built on one image, each
    differentiates straight to the renderer's inputs and the contributions add up.  If the image was edited in place
    since the renderer wrote it, the record comes back WITHOUT the renderer's empty-block map and without the loss the
    forward computed on what it wrote (the loss kernel then reads every pixel)."""
    node = image.grad_fn
    if node is None:
        return None
    try:
        record = _fused_renders.get(node)
    except TypeError:   # a built-in node (MulBackward0, ...) cannot even be weakly referenced: not ours
        return None
    if record is not None and record.get("image_version") != image._version:
        record = dict(record, empty_regions=None, l1_in_forward=None)
    return record


# The loss target's empty-block map: only for a target the caller has NAMED with losses.remember_target(target)
# (round 6).  Rounds 4-5 found the map by themselves on first use, kept it in an identity-keyed weak map and refreshed it
# every 64th use against writes that bypass the version counter: more machinery than 5 us of a 650 us step deserve.
# The map rides on the tensor object, like the adjacency on a triangle tensor, and is used while the tensor's data
# pointer, shape and version counter are what they were when it was made; anything else -- another target, an in-place
# torch write -- means no map, and the loss reads every block.  A write the counter does not see (target.data, DLPack,
# a raw kernel) after remember_target is the caller's to follow with another remember_target / forget_target.
#
# The most recently remembered target of every (device, shape) is also known to the RENDERER, by one weak reference:
# FusedPhongRenderer.forward compares an image of that shape with it inside its own pass (loss_in_forward).  A map that
# exists is refreshed IN PLACE by the next remember_target of the same tensor: a captured step (capture_step) has the
# addresses of the target and of its map baked in, and target.copy_(new); remember_target(target) must reach it.
_remembered_targets = {}   # (device, shape) -> weakref.ref(target)


def _target_key(target):
    return (target.data_ptr(), target._version, tuple(target.shape))


def remember_target_map(target):
    if target.dim() != 4 or target.shape[-1] != 4 or target.dtype != torch.float32 or not target.is_cuda:
        raise ValueError("remember_target expects a [B, H, W, 4] float32 image on the GPU")
    kept = getattr(target, "_mr_empty_regions", None)
    same_place = kept is not None and kept[0][0] == target.data_ptr() and kept[0][2] == tuple(target.shape) \
        and kept[1].device == target.device
    target._mr_empty_regions = (_target_key(target),
                                _native.image_empty_regions(target.detach(), out=kept[1] if same_place else None))
    _remembered_targets[(target.device, tuple(target.shape))] = weakref.ref(target)


def forget_target_map(target):
    if hasattr(target, "_mr_empty_regions"):
        del target._mr_empty_regions
    where = (target.device, tuple(target.shape))
    ref = _remembered_targets.get(where)
    if ref is not None and (ref() is None or ref() is target):
        del _remembered_targets[where]


def _target_empty_regions(target):
    kept = getattr(target, "_mr_empty_regions", None)
    if kept is not None and kept[0] == _target_key(target):
        return kept[1]
    return None


def _remembered_target(device, shape):
    """(target, its empty-block map) for the live remembered target of that device and shape whose key still holds --
    not edited in place, not moved -- else (None, None)."""
    ref = _remembered_targets.get((device, tuple(shape)))
    target = ref() if ref is not None else None
    if target is None:
        if ref is not None:
            del _remembered_targets[(device, tuple(shape))]
        return None, None
    empty = _target_empty_regions(target)
    if empty is None or not target.is_contiguous():
        return None, None
    return target, empty


class FusedPhongL1Loss(torch.autograd.Function):
    """mean|image - target| for an `image` that FusedPhongRenderer produced, differentiated straight
    to the renderer's inputs: the backward hands the loss's 2-bit-per-element sign codes to the
    shading backward instead of first writing -- and then re-reading -- a [B,H,W,4] float gradient
    image (losses.l1_loss routes here; same value, same gradients).

    `image` is an input of this node like any other, but in the fused mode it receives None: the chain through the
    renderer is evaluated here.  Round 5: whether anybody LOOKS at d loss / d image is decided when the backward runs
    -- retain_grad() or a tensor hook on the image (registered before or after the loss was built), or a
    torch.autograd.grad / backward(inputs=...) call that names the image (rendered_image.py) -- and the node then
    behaves exactly like the generic op: the image gets its dense gradient (formed from the sign codes), the
    renderer's own node carries it on, and this node adds nothing to the renderer's inputs itself."""

    @staticmethod
    def forward(ctx, image, target, vertices, transforms, normals, diffuse, light_positions,
                light_intensities, ambient, render_saved, prepared_state=None, empty_regions=None, l1_in_forward=None):
        # l1_in_forward (take_fused_render hands it over only for an image nobody edited): the renderer's forward already
        # compared the image with the target it knew of.  If that is THIS target, unchanged since, the loss and the sign
        # codes are taken from there and no kernel runs; any other target is compared here, as ever.
        ctx.loss_from_forward = l1_in_forward is not None and l1_in_forward["target_key"] == _target_key(target)
        if ctx.loss_from_forward:
            # (detach(): a new tensor object on the same scalar -- several losses may be built on one image)
            loss, signs = l1_in_forward["loss"].detach(), l1_in_forward["signs"]
            _native.close_pending_timer(_native.TIMER_L1_FORWARD, image.device)
        else:
            # the renderer knows which 64 x 64 blocks of its image are empty; the target's are known if the caller named it
            # (losses.remember_target): blocks empty on both sides are not read
            empty_target = _target_empty_regions(target) if empty_regions is not None else None
            loss, signs = _native.l1_loss_forward(image.detach(), target.detach(), want_signs=True,
                                                  empty_a=empty_regions, empty_b=empty_target)
        ctx.image_shape = image.shape
        ctx.prepared_state = prepared_state
        ctx.empty_regions = empty_regions
        # the image itself is SAVED (round 6; a weak reference until then): the backward looks at its retains_grad flag and
        # its hooks, and a caller that drops its own reference before backward() -- a helper that returns only the loss --
        # must not lose a hook it registered.  Freed with the graph after backward(), like any saved tensor.
        # The renderer's own saved tensors (G-buffer, corner records, adjacency, ...) are held here too, because the
        # renderer's node frees its copies as soon as the image tensor is dropped.
        ctx.save_for_backward(signs, image, *render_saved)
        return loss

    @staticmethod
    def _image_gradient_observed(image):
        from .rendered_image import image_gradient_requested
        if image_gradient_requested():
            return True
        with torch._C.DisableTorchFunctionSubclass():
            return bool(image.retains_grad or image._backward_hooks)

    @staticmethod
    def backward(ctx, grad):
        signs, image = ctx.saved_tensors[:2]
        upstream = grad.to(torch.float32).reshape(1)
        dtarget = None
        if ctx.needs_input_grad[0] and FusedPhongL1Loss._image_gradient_observed(image):
            dimage = _native.l1_loss_backward(signs, ctx.image_shape, upstream)
            if ctx.needs_input_grad[1]:
                dtarget = -dimage
            return (dimage, dtarget) + (None,) * 11
        dverts, dxf, dn, dd, _, dlp, dli, damb = FusedPhongRenderer._input_grads(
            ctx.saved_tensors[2:], ctx.needs_input_grad[3], any(ctx.needs_input_grad[6:9]), upstream,
            l1_signs=signs, needs_normal_grad=ctx.needs_input_grad[4], needs_diffuse_grad=ctx.needs_input_grad[5],
            prepared_state=ctx.prepared_state, empty_regions=ctx.empty_regions)
        if ctx.needs_input_grad[1]:
            dtarget = -_native.l1_loss_backward(signs, ctx.image_shape, upstream)
        return None, dtarget, dverts, dxf, dn, dd, dlp, dli, damb, None, None, None, None


# False (or MR_FUSE_SPECULAR_NORMS=0 at import): the specular renderer rasterizes with mr_rasterize_forward and runs the
# norm pass over the G-buffer for every group of lights (A/B, tests)
FUSE_SPECULAR_NORMS = os.environ.get("MR_FUSE_SPECULAR_NORMS", "1") != "0"


class FusedSpecularPhongRenderer(torch.autograd.Function):
    """FusedPhongRenderer plus the specular term of phong_shader (src/mesh_renderer/render.py
    :326-372): two passes over the G-buffer each way (the reference L2-normalises the
    reflection . camera dot product across all pixels of an image).  shininess is [B] (one
    exponent per image) or [B,V] (per vertex, interpolated like the other attributes) and is
    differentiated either way."""

    @staticmethod
    def forward(ctx, clip, positions, normals, diffuse, specular, triangles, light_positions,
                light_intensities, ambient, camera_position, shininess, image_width, image_height,
                transforms=None):
        """transforms ([B,4,4], not differentiated here) or None: the caller vouches that
        clip = transform_homogeneous(transforms, positions).  When the positions require a gradient and nothing
        else but `clip` does, the backward then returns the WHOLE vertex gradient as d positions and None for
        d clip (the pull-back through the transform is folded into the pixel pass)."""
        clip_d = clip.detach().contiguous()
        attrs = [t.detach().contiguous() for t in (normals, positions, diffuse, specular)]
        lp, li = light_positions.detach().contiguous(), light_intensities.detach().contiguous()
        amb = ambient.detach().contiguous() if ambient is not None else None
        cam, shin = camera_position.detach().contiguous(), shininess.detach().contiguous()
        # Round 5: the rasterizer's pass also forms the across-pixels norms of the FIRST group of lights (its tile walk
        # holds every covered pixel's normal and position): that group's norm pass over the G-buffer does not run
        first_norms = None
        if FUSE_SPECULAR_NORMS:
            ids, bary, _, first_norms = _native.rasterize_specular_norms_forward(
                clip_d, triangles, attrs[0], attrs[1], lp[:, :_native.shade_fast_lights()].contiguous(), cam,
                int(image_width), int(image_height))
        else:
            ids, bary, _ = _native.rasterize_forward(clip_d, triangles, int(image_width), int(image_height))
        # The kernels keep four lights in registers.  More (round 3): every light's term -- diffuse and
        # specular, with its own across-pixels norm -- depends on that light alone, so the image is the
        # sum of the images of groups of four lights (ambient in the first group), and the gradients
        # add up the same way in the backward.
        rgba, norms2 = None, []
        for first in range(0, lp.shape[1], _native.shade_fast_lights()):
            last = first + _native.shade_fast_lights()
            part, part_norms = _native.shade_specular_forward(
                ids, bary, attrs[0], attrs[1], attrs[2], attrs[3], triangles, lp[:, first:last].contiguous(),
                li[:, first:last].contiguous(), amb if first == 0 else None, cam, shin,
                norms2=first_norms if first == 0 else None)
            norms2.append(part_norms)
            if rgba is None:
                rgba = part
            else:
                rgba[..., :3] += part[..., :3]
        norms2 = norms2[0] if len(norms2) == 1 else torch.cat(norms2, 1)
        offsets, entries = _native.vertex_adjacency(triangles, positions.shape[1])   # cached per mesh
        saved = [clip_d, ids, bary] + attrs + [triangles, lp, li, cam, shin, norms2, offsets, entries]
        if amb is not None:
            saved.append(amb)
        ctx.has_transforms = transforms is not None
        if transforms is not None:
            saved.append(transforms.detach().to(torch.float32).contiguous())
        ctx.save_for_backward(*saved)
        ctx.has_ambient = amb is not None
        # FusedSpecularL1Loss on this image hands it NO gradient (see FusedPhongRenderer.forward)
        ctx.set_materialize_grads(False)
        # (a RenderedImage: the reference's L1 spelling on it arrives at losses.l1_loss by itself)
        from .rendered_image import wrap
        return wrap(rgba)

    @staticmethod
    def _input_grads(saved, has_ambient, has_transforms, need, upstream, l1_signs=None):
        """The specular shading backward on the tensors forward() saved -> gradients in the order of forward()'s first
        eleven arguments.  need: which of them require a gradient (same order).  l1_signs: `upstream` is then the
        scalar d L / d loss of mean|image - target| and the image gradient is that loss's sign codes
        (_native.shade_specular_backward)."""
        clip, ids, bary, normals, positions, diffuse, specular, triangles, lp, li, cam, shin, norms2 = saved[:13]
        offsets, entries = saved[13:15]
        amb = saved[15] if has_ambient else None
        transforms = saved[-1] if has_transforms else None
        # need: clip, positions, normals, diffuse, specular, -, lpos, lint, ambient, camera, shininess
        wanted = ((_native.GRAD_CLIP if need[0] else 0) | (_native.GRAD_POSITIONS if need[1] else 0)
                  | (_native.GRAD_NORMALS if need[2] else 0) | (_native.GRAD_DIFFUSE if need[3] else 0)
                  | (_native.GRAD_SPECULAR if need[4] else 0) | (_native.GRAD_SHININESS if need[10] else 0)
                  | (_native.GRAD_LIGHTS if (need[6] or need[7] or need[8] or need[9]) else 0))
        if need[10] and shin.dim() == 1:
            wanted |= _native.GRAD_LIGHTS   # the per-image exponent's gradient rides the image-wide sums
        # vertices alone: the transform's pull-back is folded in (see forward) and clip gets no gradient of its own
        fold = (transforms is not None and need[0] and need[1]
                and (wanted & ~(_native.GRAD_CLIP | _native.GRAD_POSITIONS)) == 0 and not _native.deterministic())
        if fold:
            wanted &= ~_native.GRAD_CLIP
        # per-vertex gather over the adjacency (round 3): no atomics, every output written once
        step = _native.shade_fast_lights()
        total = None
        for first in range(0, lp.shape[1], step):    # groups of four lights: see forward()
            part = _native.shade_specular_backward(
                upstream, ids, bary, clip, normals, positions, diffuse, specular, triangles,
                lp[:, first:first + step].contiguous(), li[:, first:first + step].contiguous(),
                amb if first == 0 else None, cam, shin, norms2[:, first:first + step].contiguous(),
                adjacency=(offsets, entries), transforms=transforms if fold else None, normalised_gbuffer=True,
                grads_wanted=wanted, l1_signs=l1_signs)
            if total is None:
                total = list(part)
                continue
            for k in (0, 1, 2, 3, 4, 8, 9):          # dclip, dn, dp, dd, dsp, dcam, dshin add up
                total[k] = total[k] + part[k]
            total[5] = torch.cat([total[5], part[5]], 1)   # d light_positions / d light_intensities: per light
            total[6] = torch.cat([total[6], part[6]], 1)
        dclip, dn, dp, dd, dsp, dlp, dli, damb, dcam, dshin = total
        if fold:
            dclip = None
        return dclip, dp, dn, dd, dsp, None, dlp, dli, damb, dcam, dshin

    @staticmethod
    def backward(ctx, drgba):
        if drgba is None:   # (set_materialize_grads(False): FusedSpecularL1Loss differentiated straight to the inputs)
            return (None,) * 14
        grads = FusedSpecularPhongRenderer._input_grads(ctx.saved_tensors, ctx.has_ambient, ctx.has_transforms,
                                                        ctx.needs_input_grad, drgba.contiguous())
        return grads + (None, None, None)


class FusedSpecularL1Loss(torch.autograd.Function):
    """FusedPhongL1Loss for an `image` that FusedSpecularPhongRenderer produced (round 5): mean|image - target|
    differentiated straight to the specular renderer's inputs, the backward handing the loss's sign codes to
    mr_shade_specular_backward_l1.  The one-pass vertex-gradient kernel -- the reference's optimisation loop
    (mesh_renderer_test.py:238-262) with a specular term, one or two lights -- reads the codes directly, 1 B/px
    instead of a 16 B/px gradient image written and read back; the other cases form the dense image inside the call.
    An observed d loss / d image is honoured exactly as in FusedPhongL1Loss."""

    @staticmethod
    def forward(ctx, image, target, clip, positions, normals, diffuse, specular, light_positions,
                light_intensities, ambient, camera_position, shininess, render_saved, has_ambient, has_transforms):
        loss, signs = _native.l1_loss_forward(image.detach(), target.detach(), want_signs=True)
        ctx.image_shape = image.shape
        ctx.has_ambient, ctx.has_transforms = has_ambient, has_transforms
        ctx.save_for_backward(signs, image, *render_saved)   # (the image: see FusedPhongL1Loss.forward)
        return loss

    @staticmethod
    def backward(ctx, grad):
        signs, image = ctx.saved_tensors[:2]
        upstream = grad.to(torch.float32).reshape(1)
        n = ctx.needs_input_grad
        dtarget = None
        if n[0] and FusedPhongL1Loss._image_gradient_observed(image):
            dimage = _native.l1_loss_backward(signs, ctx.image_shape, upstream)
            if n[1]:
                dtarget = -dimage
            return (dimage, dtarget) + (None,) * 13
        need = (n[2], n[3], n[4], n[5], n[6], False, n[7], n[8], n[9], n[10], n[11])
        dclip, dp, dn, dd, dsp, _, dlp, dli, damb, dcam, dshin = FusedSpecularPhongRenderer._input_grads(
            ctx.saved_tensors[2:], ctx.has_ambient, ctx.has_transforms, need, upstream, l1_signs=signs)
        if n[1]:
            dtarget = -_native.l1_loss_backward(signs, ctx.image_shape, upstream)
        return (None, dtarget, dclip, dp, dn, dd, dsp, dlp, dli, damb, dcam, dshin, None, None, None)
