"""ctypes binding of the C-ABI HIP library (include/mesh_raster.h).

This is the ONLY compute back end of the package: there is no CPU or eager
fallback.  If libmesh_raster_hip.so is missing or a tensor is not on a HIP
device, the call raises.  PyTorch supplies device memory and the stream; the
kernels are ours.
"""
import ctypes
import os
import subprocess

import torch

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# MR_NATIVE_LIB_PATH: development only (tools/raster_bench.py --variant loads the stage-timing
# build libmesh_raster_hip_probes.so this way); the product always loads the in-tree library.
LIB_PATH = os.environ.get("MR_NATIVE_LIB_PATH") or os.path.join(_CSRC, "libmesh_raster_hip.so")

ABI_VERSION = 356
GBUFFER_NORMALISED = 1   # mesh_raster.h, MR_GBUFFER_NORMALISED
GBUFFER_PRIVATE = 2      # MR_GBUFFER_PRIVATE
TIMER_RASTER_FORWARD, TIMER_SHADE_BACKWARD, TIMER_SHADE_FORWARD, TIMER_RASTER_BACKWARD, TIMER_L1_FORWARD = 0, 1, 2, 3, 4
MR_OK, MR_EINVAL, MR_EWORKSPACE, MR_ELAUNCH = 0, -1, -2, -3
_ERR = {MR_EINVAL: "invalid argument", MR_EWORKSPACE: "workspace too small or misaligned",
        MR_ELAUNCH: "HIP launch failed"}

_lib = None
_workspaces = {}
_pending_timers = {}


_deterministic = False


def set_deterministic(on):
    """Bit-reproducible gradients for the fused render / rasterize backward passes, the silhouette
    antialiasing backward (mesh_renderer.antialias) and the texture gradient of mesh_renderer.texture (see
    mr_set_deterministic in include/mesh_raster.h): fixed-point integer accumulation instead of float
    atomics, ~10 % slower.  Process-wide on the Python side: the flag is handed to the library by
    whichever thread launches a backward kernel (autograd runs them on its own thread).  Returns the
    previous setting."""
    global _deterministic
    before = _deterministic
    _deterministic = bool(on)
    return before


def deterministic():
    """Whether set_deterministic(True) is in force."""
    return _deterministic


def _sync_deterministic():
    lib().mr_set_deterministic(1 if _deterministic else 0)


# Test / measurement hook (include/mesh_raster_debug.h): pixel kernel of the shading backward --
# 0 automatic, 1 the rows kernel, 2 the lane-accumulating kernel wherever it exists.  Like the
# deterministic flag it is handed over by the launching thread.
_shade_backward_kernel = int(os.environ.get("MR_SHADE_BACKWARD_KERNEL", "0"))


def debug_set_shade_backward_kernel(which):
    global _shade_backward_kernel
    before = _shade_backward_kernel
    _shade_backward_kernel = int(which)
    return before


def debug_set_raster_repeat(n):
    """Measurement only (include/mesh_raster_debug.h): this thread's next forward calls launch k_raster n times."""
    _check(lib().mr_debug_set_raster_repeat(int(n)), "mr_debug_set_raster_repeat")


def debug_last_accumulate_kernel():
    """Tests only (include/mesh_raster_debug.h): the functor of the most recent backward pixel pass any thread
    launched, e.g. 'ShadeFoldLaneFn<1, true>' ('' before the first)."""
    text = lib().mr_debug_last_accumulate_kernel().decode()
    return text.split("Fn = mr::")[-1].rstrip("]").replace("(anonymous namespace)::", "") if "Fn = " in text else text


def debug_set_lanes_rows(rows):
    """Tests only (include/mesh_raster_debug.h): strip height of the lane-accumulating pixel pass for THIS thread's next
    launches -- 0 automatic (default), 4 / 8 / 16 forced."""
    _check(lib().mr_debug_set_lanes_rows(int(rows)), "mr_debug_set_lanes_rows")


def debug_last_lanes_rows():
    """Tests only: strip height the most recent lane-accumulating launch used (0 before the first)."""
    return int(lib().mr_debug_last_lanes_rows())


def debug_soft_nearest(points, seg_a, seg_b):
    """Tests only (include/mesh_raster_debug.h): the SoftRas kernels' nearest-point-on-a-segment
    evaluation for [n,2] device points / segment ends -> [n,4] = (nearest x, y, t, squared distance)."""
    for name, t in (("points", points), ("seg_a", seg_a), ("seg_b", seg_b)):
        _chk(name, t, _F32, None, 2)
    if not (points.shape == seg_a.shape == seg_b.shape):
        raise ValueError("points, seg_a and seg_b must have the same [n,2] shape")
    dev = _require_device(points, seg_a, seg_b)
    out = torch.empty(points.shape[0], 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib().mr_debug_soft_nearest(_ptr(points.contiguous()), _ptr(seg_a.contiguous()), _ptr(seg_b.contiguous()),
                                         points.shape[0], _ptr(out), _stream(dev))
    _check(rc, "mr_debug_soft_nearest")
    return out


def time_next_kernel(which, start_event, stop_event):
    """Measurement (bench.py): HIP events (ctypes.c_void_p) to record around the NEXT launch of
    kernel `which` (TIMER_*) made through this module, from whatever thread makes it -- autograd runs
    backward passes on its own thread, and the library's one-shot timers are per thread, so the pair
    is handed to mr_time_next_kernel by the launching wrapper itself."""
    _pending_timers[which] = (start_event, stop_event)


def _arm_timer(which):
    pair = _pending_timers.pop(which, None)
    if pair is not None:
        lib().mr_time_next_kernel(which, pair[0], pair[1])


def close_pending_timer(which, dev):
    """A pair handed to time_next_kernel whose kernel will not run in this step (the loss that the fused forward already
    computed): left pending, it would bracket some LATER launch of that kernel and be read as this step's.  It is
    recorded back to back on the current stream instead -- an empty interval: whoever reads the pair finds recorded
    events and (nearly) zero, not events that never happened (hipEventElapsedTime fails on those, and the error stays
    behind as the thread's last HIP error for the next caller that looks)."""
    pair = _pending_timers.pop(which, None)
    if pair is not None:
        with torch.cuda.device(dev):
            lib().mr_time_next_kernel(which, pair[0], pair[1])
            lib().mr_time_no_kernel(which, _stream(dev))



class NativeLibraryError(RuntimeError):
    pass


def build(verbose=False):
    """Compile libmesh_raster_hip.so in-tree for gfx950 (hipcc cross-compiles on CPU)."""
    out = subprocess.run(["make", "-C", _CSRC, "all"], capture_output=True, text=True)
    if verbose:
        print(out.stdout)
    if out.returncode != 0:
        raise NativeLibraryError("hipcc build failed:\n" + out.stdout + out.stderr)
    return LIB_PATH


def lib():
    """Load the shared library (never builds implicitly, never falls back)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                "%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or make -C pytorch_mesh_renderer_amd/csrc). There is no fallback path." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        L.mr_version.restype = ci
        if L.mr_version() != ABI_VERSION:   # a stale .so would be called with the wrong signatures
            raise NativeLibraryError("%s has ABI version %d, this package needs %d: rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, L.mr_version(), ABI_VERSION))
        L.mr_last_hip_error.restype = ci
        L.mr_set_deterministic.argtypes = [ci]
        L.mr_set_deterministic.restype = ci
        L.mr_time_next_kernel.argtypes = [ci, vp, vp]
        L.mr_time_next_kernel.restype = ci
        # include/mesh_raster_debug.h (tests and tools only)
        L.mr_debug_set_raster_probe.argtypes = [ci]
        L.mr_debug_set_raster_probe.restype = ci
        L.mr_debug_set_raster_region_edge.argtypes = [ci]
        L.mr_debug_set_raster_region_edge.restype = ci
        L.mr_debug_set_shade_backward_kernel.argtypes = [ci]
        L.mr_debug_set_shade_backward_kernel.restype = ci
        L.mr_debug_set_raster_repeat.argtypes = [ci]
        L.mr_debug_set_raster_repeat.restype = ci
        L.mr_debug_last_accumulate_kernel.argtypes = []
        L.mr_debug_last_accumulate_kernel.restype = ctypes.c_char_p
        L.mr_debug_set_lanes_rows.argtypes = [ci]
        L.mr_debug_set_lanes_rows.restype = ci
        L.mr_debug_last_lanes_rows.argtypes = []
        L.mr_debug_last_lanes_rows.restype = ci
        L.mr_debug_soft_nearest.argtypes = [vp, vp, vp, ci, vp, vp]
        L.mr_debug_soft_nearest.restype = ci
        L.mr_rasterize_forward_workspace_bytes.argtypes = [ci] * 5
        L.mr_rasterize_forward_workspace_bytes.restype = sz
        L.mr_rasterize_forward.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]
        L.mr_rasterize_forward.restype = ci
        L.mr_rasterize_backward_workspace_bytes.argtypes = [ci] * 5
        L.mr_rasterize_backward_workspace_bytes.restype = sz
        L.mr_rasterize_backward.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, sz, vp]
        L.mr_rasterize_backward.restype = ci
        L.mr_interpolate_forward.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]
        L.mr_interpolate_forward.restype = ci
        L.mr_interpolate_backward_workspace_bytes.argtypes = [ci] * 6
        L.mr_interpolate_backward_workspace_bytes.restype = sz
        L.mr_interpolate_backward.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci,
                                              vp, vp, vp, sz, vp]
        L.mr_interpolate_backward.restype = ci
        L.mr_shade_max_lights.restype = ci
        L.mr_shade_fast_lights.argtypes = []
        L.mr_shade_fast_lights.restype = ci
        L.mr_shade_forward_workspace_bytes.argtypes = [ci] * 5
        L.mr_shade_forward_workspace_bytes.restype = sz
        L.mr_shade_forward.argtypes = [vp] * 9 + [ci] * 6 + [vp, vp, sz, vp]
        L.mr_shade_forward.restype = ci
        L.mr_shade_backward_workspace_bytes.argtypes = [ci] * 5
        L.mr_shade_backward_workspace_bytes.restype = sz
        L.mr_shade_backward_prepared_bytes.argtypes = [ci] * 2
        L.mr_shade_backward_prepared_bytes.restype = sz
        L.mr_shade_backward.argtypes = [vp] * 11 + [ci] * 6 + [vp] * 9 + [ci, vp, vp, vp, sz, vp]
        L.mr_shade_backward.restype = ci
        L.mr_shade_backward_l1_workspace_bytes.argtypes = [ci] * 5
        L.mr_shade_backward_l1_workspace_bytes.restype = sz
        L.mr_shade_backward_l1.argtypes = [vp] * 12 + [ci] * 6 + [vp] * 9 + [ci, vp, vp, vp, sz, vp]
        L.mr_shade_backward_l1.restype = ci
        L.mr_soft_max_lights.restype = ci
        L.mr_soft_workspace_bytes.argtypes = [ci] * 5
        L.mr_soft_workspace_bytes.restype = sz
        cf = ctypes.c_float
        L.mr_soft_forward.argtypes = [vp] * 7 + [ci] * 6 + [cf] * 3 + [vp, vp, vp, sz, vp]
        L.mr_soft_forward.restype = ci
        L.mr_soft_prepared_bytes.argtypes = [ci] * 5
        L.mr_soft_prepared_bytes.restype = sz
        L.mr_soft_backward.argtypes = [vp] * 10 + [ci] * 6 + [cf] * 3 + [vp] * 6 + [vp, vp, sz, vp]
        L.mr_soft_backward.restype = ci
        fp = vp
        L.mr_camera_transforms.argtypes = [fp, fp, fp, fp, fp, fp, ctypes.c_float, ci, fp, vp, vp]
        L.mr_camera_transforms.restype = ci
        L.mr_camera_transforms_backward.argtypes = [fp, fp, fp, fp, fp, fp, fp, ctypes.c_float, ci, fp, fp, fp, vp]
        L.mr_camera_transforms_backward.restype = ci
        L.mr_l1_loss_partials.argtypes = []
        L.mr_l1_loss_partials.restype = ci
        L.mr_l1_loss_forward.argtypes = [vp, vp, sz, vp, vp, vp, vp]
        L.mr_l1_loss_forward.restype = ci
        L.mr_l1_loss_backward.argtypes = [vp, sz, vp, vp, vp]
        L.mr_l1_loss_backward.restype = ci
        L.mr_interpolate_raster_max_attributes.restype = ci
        L.mr_interpolate_raster_backward_workspace_bytes.argtypes = [ci] * 6
        L.mr_interpolate_raster_backward_workspace_bytes.restype = sz
        L.mr_interpolate_records_bytes.argtypes = [ci] * 3
        L.mr_interpolate_records_bytes.restype = sz
        L.mr_interpolate_forward_records.argtypes = [vp] * 5 + [ci] * 6 + [vp, vp, sz, vp]
        L.mr_interpolate_forward_records.restype = ci
        L.mr_rasterize_interpolate_forward.argtypes = [vp] * 4 + [ci] * 6 + [vp] * 5 + [sz, vp, sz, vp]
        L.mr_rasterize_interpolate_forward.restype = ci
        L.mr_interpolate_raster_backward.argtypes = [vp] * 10 + [ci] * 6 + [vp, vp, ci, vp, sz, vp]
        L.mr_interpolate_raster_backward.restype = ci
        L.mr_vertex_transform.argtypes = [vp, vp, ci, ci, vp, vp]
        L.mr_vertex_transform.restype = ci
        L.mr_render_forward.argtypes = [vp] * 8 + [ci] * 6 + [vp, vp, vp, vp, ci] + [vp] * 6 + [sz, vp]
        L.mr_empty_regions_bytes.argtypes = [ci] * 3
        L.mr_empty_regions_bytes.restype = sz
        L.mr_image_empty_regions.argtypes = [vp, ci, ci, ci, vp, vp]
        L.mr_image_empty_regions.restype = ci
        L.mr_l1_loss_forward_regions.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp]
        L.mr_l1_loss_forward_regions.restype = ci
        L.mr_render_forward.restype = ci
        L.mr_shade_specular_forward_workspace_bytes.argtypes = [ci] * 5
        L.mr_shade_specular_forward_workspace_bytes.restype = sz
        L.mr_shade_specular_forward.argtypes = [vp] * 12 + [ci] * 7 + [vp, vp, ci, vp, sz, vp]
        L.mr_shade_specular_forward.restype = ci
        L.mr_rasterize_specular_norms_workspace_bytes.argtypes = [ci] * 5
        L.mr_rasterize_specular_norms_workspace_bytes.restype = sz
        L.mr_rasterize_specular_norms_forward.argtypes = [vp] * 6 + [ci] * 6 + [vp, vp, vp, ci, vp, vp, sz, vp]
        L.mr_rasterize_specular_norms_forward.restype = ci
        L.mr_shade_specular_backward_workspace_bytes.argtypes = [ci] * 5
        L.mr_shade_specular_backward_workspace_bytes.restype = sz
        L.mr_shade_specular_backward.argtypes = [vp] * 14 + [ci, vp] + [ci] * 6 + [vp] * 7 + [vp, vp] + [vp, ci, ci] + [vp, sz, vp]
        L.mr_shade_specular_backward.restype = ci
        L.mr_shade_specular_backward_l1_workspace_bytes.argtypes = [ci] * 5
        L.mr_shade_specular_backward_l1_workspace_bytes.restype = sz
        L.mr_shade_specular_backward_l1.argtypes = [vp] * 15 + [ci, vp] + [ci] * 6 + [vp] * 7 + [vp, vp] + [vp, ci, ci] + [vp, sz, vp]
        L.mr_shade_specular_backward_l1.restype = ci
        L.mr_export_u8.argtypes = [vp, sz, vp, vp]
        L.mr_export_u8.restype = ci
        L.mr_tone_map.argtypes = [vp, ci, sz, cf, vp, vp, vp, vp]
        L.mr_tone_map.restype = ci
        L.mr_vertex_normals_forward.argtypes = [vp] * 4 + [ci] * 3 + [vp, vp, vp]
        L.mr_vertex_normals_forward.restype = ci
        L.mr_vertex_normals_backward.argtypes = [vp] * 6 + [ci] * 3 + [vp, vp]
        L.mr_vertex_normals_backward.restype = ci
        L.mr_antialias_forward.argtypes = [vp] * 7 + [ci] * 6 + [vp, vp, vp]
        L.mr_antialias_forward.restype = ci
        L.mr_antialias_backward_workspace_bytes.argtypes = [ci] * 6
        L.mr_antialias_backward_workspace_bytes.restype = sz
        L.mr_antialias_backward.argtypes = [vp] * 8 + [ci] * 6 + [vp, vp, vp, sz, vp]
        L.mr_antialias_backward.restype = ci
        L.mr_sh_shade_forward.argtypes = [vp, vp, ci, vp, vp, ci, ci, ci, ci, vp, vp]
        L.mr_sh_shade_forward.restype = ci
        L.mr_sh_shade_backward_workspace_bytes.argtypes = [ci] * 3
        L.mr_sh_shade_backward_workspace_bytes.restype = sz
        L.mr_sh_shade_backward.argtypes = [vp, vp, vp, ci, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, sz, vp]
        L.mr_sh_shade_backward.restype = ci
        try:
            L.mr_texture_forward.argtypes = [vp] * 3 + [ci] * 8 + [vp, vp]
            L.mr_texture_forward.restype = ci
            L.mr_texture_backward_workspace_bytes.argtypes = [ci] * 7
            L.mr_texture_backward_workspace_bytes.restype = sz
            L.mr_texture_backward.argtypes = [vp] * 4 + [ci] * 8 + [vp, vp, vp, sz, vp]
            L.mr_texture_backward.restype = ci
            L.mr_texture_mip_levels.argtypes = [ci] * 3
            L.mr_texture_mip_levels.restype = ci
            L.mr_texture_mip_pyramid_bytes.argtypes = [ci] * 6
            L.mr_texture_mip_pyramid_bytes.restype = sz
            L.mr_texture_mip_forward.argtypes = [vp] * 4 + [ci] * 9 + [vp, vp, vp]
            L.mr_texture_mip_forward.restype = ci
            L.mr_texture_mip_backward_workspace_bytes.argtypes = [ci] * 8
            L.mr_texture_mip_backward_workspace_bytes.restype = sz
            L.mr_texture_mip_backward.argtypes = [vp] * 6 + [ci] * 9 + [vp, vp, vp, sz, vp]
            L.mr_texture_mip_backward.restype = ci
            L.mr_attribute_derivatives.argtypes = [vp] * 6 + [ci] * 7 + [vp, vp]
            L.mr_attribute_derivatives.restype = ci
        except AttributeError as e:   # the texture entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the texture entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_render_forward_l1_partials.argtypes = [ci] * 3
            L.mr_render_forward_l1_partials.restype = sz
            L.mr_render_forward_l1.argtypes = L.mr_render_forward.argtypes + [vp] * 5
            L.mr_render_forward_l1.restype = ci
            L.mr_time_no_kernel.argtypes = [ci, vp]
            L.mr_time_no_kernel.restype = ci
        except AttributeError as e:   # the loss-in-forward entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks mr_render_forward_l1 (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_render_forward_l1_private_bytes.argtypes = [ci] * 4
            L.mr_render_forward_l1_private_bytes.restype = sz
            # mr_render_forward_l1 without `bary` and `want_z`
            L.mr_render_forward_l1_private.argtypes = [vp] * 8 + [ci] * 6 + [vp] * 9 + [sz, vp] + [vp] * 5
            L.mr_render_forward_l1_private.restype = ci
        except AttributeError as e:   # the private G-buffer entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks mr_render_forward_l1_private (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_mesh_regularizer_workspace_bytes.argtypes = [ci] * 3
            L.mr_mesh_regularizer_workspace_bytes.restype = sz
            L.mr_mesh_regularizer_forward.argtypes = [vp] * 4 + [ci] * 6 + [cf, vp, vp, vp, sz, vp]
            L.mr_mesh_regularizer_forward.restype = ci
            L.mr_mesh_regularizer_backward.argtypes = [vp] * 8 + [ci] * 6 + [cf, vp, vp]
            L.mr_mesh_regularizer_backward.restype = ci
        except AttributeError as e:   # the regulariser entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the mesh regulariser entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_ssim_partials.argtypes = [ci] * 5
            L.mr_ssim_partials.restype = sz
            L.mr_ssim_saved_floats.argtypes = [ci] * 7
            L.mr_ssim_saved_floats.restype = sz
            L.mr_ssim_forward.argtypes = [vp, vp] + [ci] * 5 + [cf] * 3 + [ci, ci] + [vp] * 5
            L.mr_ssim_forward.restype = ci
            L.mr_ssim_backward.argtypes = [vp] * 4 + [ci] * 5 + [cf, ci, ci, vp, vp, vp]
            L.mr_ssim_backward.restype = ci
        except AttributeError as e:   # the SSIM entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the SSIM entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_nearest_plan.argtypes = [ci] * 3 + [vp] * 4
            L.mr_nearest_plan.restype = ci
            L.mr_nearest_workspace_bytes.argtypes = [ci] * 3
            L.mr_nearest_workspace_bytes.restype = sz
            L.mr_nearest_forward.argtypes = [vp] * 4 + [ci] * 3 + [vp, vp, vp, cf, ci, vp, sz, vp]
            L.mr_nearest_forward.restype = ci
            L.mr_nearest_backward.argtypes = [vp] * 4 + [ci] * 3 + [vp] * 8 + [cf, cf, vp, vp, vp]
            L.mr_nearest_backward.restype = ci
        except AttributeError as e:   # the point-cloud entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the nearest-neighbour entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_nearest_triangle_plan.argtypes = [ci] * 3 + [vp] * 4
            L.mr_nearest_triangle_plan.restype = ci
            L.mr_nearest_triangle_workspace_bytes.argtypes = [ci] * 3
            L.mr_nearest_triangle_workspace_bytes.restype = sz
            L.mr_nearest_triangle_forward.argtypes = [vp] * 4 + [ci] * 4 + [vp] * 5 + [sz, vp]
            L.mr_nearest_triangle_forward.restype = ci
            L.mr_nearest_triangle_backward.argtypes = [vp] * 4 + [ci] * 4 + [vp] * 9
            L.mr_nearest_triangle_backward.restype = ci
        except AttributeError as e:   # the point-to-mesh entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the nearest-triangle entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_nearest_point_of_triangle_plan.argtypes = [ci] * 3 + [vp] * 4
            L.mr_nearest_point_of_triangle_plan.restype = ci
            L.mr_nearest_point_of_triangle_workspace_bytes.argtypes = [ci] * 3
            L.mr_nearest_point_of_triangle_workspace_bytes.restype = sz
            L.mr_nearest_point_of_triangle_forward.argtypes = [vp] * 4 + [ci] * 4 + [vp] * 6 + [sz, vp]
            L.mr_nearest_point_of_triangle_forward.restype = ci
            L.mr_nearest_point_of_triangle_backward.argtypes = [vp] * 4 + [ci] * 4 + [vp] * 12
            L.mr_nearest_point_of_triangle_backward.restype = ci
        except AttributeError as e:   # the mesh-to-point entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the nearest-point-of-triangle entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_knn_plan.argtypes = [ci] * 4 + [vp] * 5
            L.mr_knn_plan.restype = ci
            L.mr_knn_workspace_bytes.argtypes = [ci] * 4
            L.mr_knn_workspace_bytes.restype = sz
            L.mr_knn_forward.argtypes = [vp] * 4 + [ci] * 4 + [vp, vp, vp, sz, vp]
            L.mr_knn_forward.restype = ci
            L.mr_knn_backward.argtypes = [vp] * 4 + [ci] * 4 + [vp] * 8
            L.mr_knn_backward.restype = ci
        except AttributeError as e:   # the K-nearest-neighbour entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the K-nearest-neighbour entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_farthest_plan.argtypes = [ci] * 3 + [vp] * 4
            L.mr_farthest_plan.restype = ci
            L.mr_farthest_workspace_bytes.argtypes = [ci] * 3
            L.mr_farthest_workspace_bytes.restype = sz
            L.mr_farthest_forward.argtypes = [vp] * 3 + [ci] * 4 + [vp, vp, vp, sz, vp]
            L.mr_farthest_forward.restype = ci
            L.mr_debug_set_farthest_shape.argtypes = [ci, ci]
            L.mr_debug_set_farthest_shape.restype = ci
        except AttributeError as e:   # the farthest-point entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the farthest-point sampling entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_laplacian_apply.argtypes = [vp] * 3 + [ci] * 4 + [cf, vp, vp]
            L.mr_laplacian_apply.restype = ci
            L.mr_laplacian_solve_plan.argtypes = [ci] * 3 + [vp] * 4
            L.mr_laplacian_solve_plan.restype = ci
            L.mr_laplacian_solve_workspace_bytes.argtypes = [ci] * 3
            L.mr_laplacian_solve_workspace_bytes.restype = sz
            L.mr_laplacian_solve.argtypes = ([vp] * 4 + [ci] * 4 + [cf, ctypes.c_double] + [ci] * 4 + [vp] * 5
                                             + [sz, vp])
            L.mr_laplacian_solve.restype = ci
        except AttributeError as e:   # the Laplacian solve entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the Laplacian solve entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_align_workspace_bytes.argtypes = [ci, ci]
            L.mr_align_workspace_bytes.restype = sz
            L.mr_align_solve.argtypes = ([vp, vp, vp, ci, vp, vp, cf, vp] + [ci] * 5 + [ctypes.c_double] + [vp] * 8
                                         + [sz, vp])
            L.mr_align_solve.restype = ci
            L.mr_align_apply.argtypes = [vp] * 5 + [ci, ci, vp, vp]
            L.mr_align_apply.restype = ci
            L.mr_align_closest_points.argtypes = [vp] * 4 + [ci] * 4 + [vp, vp]
            L.mr_align_closest_points.restype = ci
            L.mr_align_icp_init.argtypes = [vp] * 3 + [ci] + [vp] * 8
            L.mr_align_icp_init.restype = ci
        except AttributeError as e:   # the registration entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the registration entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_winding_number_plan.argtypes = [ci] * 3 + [vp] * 4
            L.mr_winding_number_plan.restype = ci
            L.mr_winding_number_workspace_bytes.argtypes = [ci] * 3
            L.mr_winding_number_workspace_bytes.restype = sz
            L.mr_winding_number_forward.argtypes = [vp] * 4 + [ci] * 4 + [vp, vp, sz, vp]
            L.mr_winding_number_forward.restype = ci
        except AttributeError as e:   # the winding-number entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the winding-number entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        try:
            L.mr_cast_rays_plan.argtypes = [ci] * 3 + [vp] * 4
            L.mr_cast_rays_plan.restype = ci
            L.mr_cast_rays_workspace_bytes.argtypes = [ci] * 3
            L.mr_cast_rays_workspace_bytes.restype = sz
            L.mr_cast_rays_forward.argtypes = [vp] * 5 + [ci] * 4 + [cf, cf] + [vp] * 4 + [sz, vp]
            L.mr_cast_rays_forward.restype = ci
            L.mr_cast_rays_backward.argtypes = [vp] * 4 + [ci] * 4 + [vp] * 10
            L.mr_cast_rays_backward.restype = ci
        except AttributeError as e:   # the ray-casting entry points came without an ABI version bump
            raise NativeLibraryError("%s lacks the ray-casting entry points (%s): rebuild it (make -C "
                                     "pytorch_mesh_renderer_amd/csrc)" % (LIB_PATH, e))
        _lib = L
    return _lib


def _check(rc, what):
    if rc != MR_OK:
        extra = ""
        if rc == MR_ELAUNCH:
            extra = " (hipError %d)" % lib().mr_last_hip_error()
        raise RuntimeError("%s failed: %s%s" % (what, _ERR.get(rc, "error %d" % rc), extra))


def _require_device(*tensors):
    dev = tensors[0].device
    if dev.type != "cuda":
        raise RuntimeError(
            "pytorch_mesh_renderer_amd runs on MI355X only: got a %s tensor. Move inputs to "
            "a HIP device ('cuda'); there is no CPU fallback." % dev.type)
    for t in tensors:
        if t.device != dev:
            raise RuntimeError("all tensors must be on the same device")
    return dev


def _chk(name, t, dtype, *shape):
    """One argument of a C-ABI call: dtype as the reference's accessor<> demands (RuntimeError, like
    c10::Error there), rank and extents as the call's other arguments imply (ValueError, like the
    reference's Python layer).  The library takes raw device pointers: a tensor of another dtype or
    shape would be read as garbage or out of bounds, so NOTHING reaches it unchecked.  None in
    `shape` = any extent."""
    if not torch.is_tensor(t):
        raise TypeError("%s must be a tensor" % name)
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s, got %s" % (name, str(dtype).replace("torch.", ""),
                                                      str(t.dtype).replace("torch.", "")))
    if t.dim() != len(shape) or any(want is not None and want != have for want, have in zip(shape, t.shape)):
        raise ValueError("%s must have shape [%s], got %s" % (
            name, ", ".join("*" if d is None else str(d) for d in shape), list(t.shape)))


_F32, _I32, _U8 = torch.float32, torch.int32, torch.uint8


def _chk_mesh(clip, triangles):
    _chk("clip-space vertices", clip, _F32, None, None, 4)
    _chk("triangles", triangles, _I32, None, 3)
    return clip.shape[0], clip.shape[1], triangles.shape[0]


def _chk_gbuffer(ids, bary, B):
    _chk("triangle ids", ids, _I32, B, None, None)
    _chk("barycentrics", bary, _F32, B, ids.shape[1], ids.shape[2], 3)
    return ids.shape[1], ids.shape[2]


def _chk_lights(light_positions, light_intensities, ambient, B, max_lights):
    _chk("light_positions", light_positions, _F32, B, None, 3)
    L = light_positions.shape[1]
    if not 1 <= L <= max_lights:
        raise ValueError("1..%d lights are supported, got %d" % (max_lights, L))
    _chk("light_intensities", light_intensities, _F32, B, L, 3)
    if ambient is not None:
        _chk("ambient_color", ambient, _F32, B, 3)
    return L


def _chk_shininess(shininess, B, V):
    """[B] -> False (one exponent per image), [B,V] -> True (per vertex)."""
    if torch.is_tensor(shininess) and shininess.dim() == 2:
        _chk("shininess", shininess, _F32, B, V)
        return True
    _chk("shininess", shininess, _F32, B)
    return False


_WORKSPACE_LIMIT_BYTES = 64 << 30   # refuse absurd scratch requests instead of trying to allocate them


def _workspace(dev, nbytes):
    """Per-(device, stream) scratch tensor, grown on demand.  Reuse is safe because every consumer is
    enqueued on the same stream.  While a stream is being captured into a HIP graph the scratch comes
    from the capture's own memory pool and is NOT cached: a tensor of that pool must not outlive the
    graph or be handed to eager launches.  At most one buffer per (device, stream) is kept; a
    request beyond _WORKSPACE_LIMIT_BYTES (sizes: INTEGRATION.md, "Scratch memory") is an error."""
    if nbytes == 0:
        return None, 0
    if nbytes > _WORKSPACE_LIMIT_BYTES:
        raise RuntimeError("this call needs %.1f GiB of scratch memory (limit %.0f GiB): split the batch"
                           % (nbytes / 2.0 ** 30, _WORKSPACE_LIMIT_BYTES / 2.0 ** 30))
    if torch.cuda.is_current_stream_capturing():
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return ws, ws.numel()
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
        _workspaces[key] = ws
    return ws, ws.numel()


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def rasterize_forward(clip, triangles, width, height):
    """clip [B,V,4] f32, triangles [T,3] i32 (device) -> ids [B,H,W] i32, bary [B,H,W,3], z [B,H,W]."""
    _chk_mesh(clip, triangles)
    dev = _require_device(clip, triangles)
    L = lib()
    clip = clip.contiguous()
    triangles = triangles.contiguous()
    B, V, _ = clip.shape
    T = triangles.shape[0]
    ids = torch.empty(B, height, width, dtype=torch.int32, device=dev)
    bary = torch.empty(B, height, width, 3, dtype=torch.float32, device=dev)
    z = torch.empty(B, height, width, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        need = L.mr_rasterize_forward_workspace_bytes(B, V, T, width, height)
        ws, have = _workspace(dev, need)
        _arm_timer(TIMER_RASTER_FORWARD)
        rc = L.mr_rasterize_forward(_ptr(clip), _ptr(triangles), B, V, T, width, height,
                                    _ptr(ids), _ptr(bary), _ptr(z), _ptr(ws), have, _stream(dev))
    _check(rc, "mr_rasterize_forward")
    return ids, bary, z


def rasterize_backward(dbary, clip, triangles, ids, bary):
    """-> dclip [B,V,4] f32."""
    B, _, _ = _chk_mesh(clip, triangles)
    h, w = _chk_gbuffer(ids, bary, B)
    _chk("df_dbarycentric_coords", dbary, _F32, B, h, w, 3)
    dev = _require_device(dbary, clip, triangles, ids, bary)
    L = lib()
    dbary, clip, triangles = dbary.contiguous(), clip.contiguous(), triangles.contiguous()
    ids, bary = ids.contiguous(), bary.contiguous()
    B, V, _ = clip.shape
    T = triangles.shape[0]
    _, H, W = ids.shape
    dclip = torch.empty(B, V, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        need = L.mr_rasterize_backward_workspace_bytes(B, V, T, W, H)
        ws, have = _workspace(dev, need)
        _arm_timer(TIMER_RASTER_BACKWARD)
        _sync_deterministic()
        rc = L.mr_rasterize_backward(_ptr(dbary), _ptr(clip), _ptr(triangles), _ptr(ids),
                                     _ptr(bary), B, V, T, W, H, _ptr(dclip), _ptr(ws), have,
                                     _stream(dev))
    _check(rc, "mr_rasterize_backward")
    return dclip


def interpolate_forward(ids, bary, attrs, triangles, background):
    """attrs [B,V,A], background [A] -> [B,H,W,A]."""
    _chk("triangles", triangles, _I32, None, 3)
    _chk("attributes", attrs, _F32, None, None, None)
    _chk_gbuffer(ids, bary, attrs.shape[0])
    _chk("background", background, _F32, attrs.shape[2])
    dev = _require_device(ids, bary, attrs, triangles, background)
    L = lib()
    ids, bary, attrs = ids.contiguous(), bary.contiguous(), attrs.contiguous()
    triangles, background = triangles.contiguous(), background.contiguous()
    B, H, W = ids.shape
    V, A = attrs.shape[1], attrs.shape[2]
    T = triangles.shape[0]
    out = torch.empty(B, H, W, A, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = L.mr_interpolate_forward(_ptr(ids), _ptr(bary), _ptr(attrs), _ptr(triangles),
                                      _ptr(background), B, V, T, W, H, A, _ptr(out), _stream(dev))
    _check(rc, "mr_interpolate_forward")
    return out


def interpolate_backward(dout, ids, bary, attrs, triangles, background):
    """-> (dattrs [B,V,A], dbary [B,H,W,3])."""
    _chk("triangles", triangles, _I32, None, 3)
    _chk("attributes", attrs, _F32, None, None, None)
    h, w = _chk_gbuffer(ids, bary, attrs.shape[0])
    _chk("background", background, _F32, attrs.shape[2])
    _chk("upstream gradient", dout, _F32, attrs.shape[0], h, w, attrs.shape[2])
    dev = _require_device(dout, ids, bary, attrs, triangles, background)
    L = lib()
    dout, ids, bary = dout.contiguous(), ids.contiguous(), bary.contiguous()
    attrs, triangles, background = attrs.contiguous(), triangles.contiguous(), background.contiguous()
    B, H, W = ids.shape
    V, A = attrs.shape[1], attrs.shape[2]
    T = triangles.shape[0]
    dattrs = torch.empty(B, V, A, dtype=torch.float32, device=dev)
    dbary = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        need = L.mr_interpolate_backward_workspace_bytes(B, V, T, W, H, A)
        ws, have = _workspace(dev, need)
        rc = L.mr_interpolate_backward(_ptr(dout), _ptr(ids), _ptr(bary), _ptr(attrs),
                                       _ptr(triangles), _ptr(background), B, V, T, W, H, A,
                                       _ptr(dattrs), _ptr(dbary), _ptr(ws), have, _stream(dev))
    _check(rc, "mr_interpolate_backward")
    return dattrs, dbary


def shade_max_lights():
    return int(lib().mr_shade_max_lights())


def shade_fast_lights():
    """Lights per call of the specular kernels and of the light gradients (kept in registers)."""
    return int(lib().mr_shade_fast_lights())


def _aligned_bytes(nbytes, dev):
    """A fresh uint8 tensor of `nbytes` whose data pointer is 256-byte aligned."""
    raw = torch.empty(max(int(nbytes), 1) + 256, dtype=torch.uint8, device=dev)
    off = (-raw.data_ptr()) % 256
    return raw[off:off + max(int(nbytes), 1)]


def shade_forward(ids, bary, normals, positions, diffuse, triangles, light_positions,
                  light_intensities, ambient, keep_corner_records=False):
    """Fused interpolation + diffuse/ambient Phong: -> rgba [B,H,W,4] (row 0 = top); with
    keep_corner_records also the gathered per-triangle attribute records, for shade_backward."""
    tensors = [ids, bary, normals, positions, diffuse, triangles, light_positions, light_intensities]
    _chk("triangles", triangles, _I32, None, 3)
    _chk("positions", positions, _F32, None, None, 3)
    B, V = positions.shape[0], positions.shape[1]
    _chk("normals", normals, _F32, B, V, 3)
    _chk("diffuse colors", diffuse, _F32, B, V, 3)
    _chk_gbuffer(ids, bary, B)
    _chk_lights(light_positions, light_intensities, ambient, B, shade_max_lights())
    dev = _require_device(*(tensors + ([ambient] if ambient is not None else [])))
    L = lib()
    ids, bary, normals, positions, diffuse, triangles, light_positions, light_intensities = [
        t.contiguous() for t in tensors]
    ambient = ambient.contiguous() if ambient is not None else None
    B, H, W = ids.shape
    V, T, nl = normals.shape[1], triangles.shape[0], light_positions.shape[1]
    rgba = torch.empty(B, H, W, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        need = L.mr_shade_forward_workspace_bytes(B, V, T, W, H)
        if keep_corner_records:   # own buffer (not the shared workspace): handed to the backward
            ws, have = _aligned_bytes(need, dev), need
        else:
            ws, have = _workspace(dev, need)
        _arm_timer(TIMER_SHADE_FORWARD)
        rc = L.mr_shade_forward(_ptr(ids), _ptr(bary), _ptr(normals), _ptr(positions), _ptr(diffuse),
                                _ptr(triangles), _ptr(light_positions), _ptr(light_intensities),
                                _ptr(ambient), B, V, T, W, H, nl, _ptr(rgba), _ptr(ws), have,
                                _stream(dev))
    _check(rc, "mr_shade_forward")
    return (rgba, ws) if keep_corner_records else rgba


def vertex_transform(vertices, transforms):
    """clip [B,V,4] = transforms [B,4,4] . (vertices [B,V,3], 1), as render_forward forms it."""
    _chk("vertices", vertices, _F32, None, None, 3)
    B, V = vertices.shape[0], vertices.shape[1]
    _chk("clip-space transforms", transforms, _F32, B, 4, 4)
    dev = _require_device(vertices, transforms)
    vertices, transforms = vertices.contiguous(), transforms.contiguous()
    clip = torch.empty(B, V, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib().mr_vertex_transform(_ptr(vertices), _ptr(transforms), B, V, _ptr(clip), _stream(dev))
    _check(rc, "mr_vertex_transform")
    return clip


def render_forward(vertices, transforms, normals, diffuse, triangles, light_positions, light_intensities,
                   ambient, width, height, want_z=True, want_u8=False, prepare_backward=False, want_empty_regions=False,
                   l1_target=None, l1_target_empty=None, private_gbuffer=False):
    """render()'s forward from world-space vertices: clip-space transform, rasterizer and shading
    (the shading is the epilogue of the rasterizer's tile walk: one pass over the pixels)
    -> (clip, ids, bary, z, rgba, corner_records); with want_z=False the depth plane is not written
    (z is returned as None); with want_u8=True a seventh value follows, the image as [B,H,W,4] uint8
    frames (what export_u8(rgba) would return).

    prepare_backward=True (the caller will differentiate to the world-space vertices only): the setup kernel
    also writes the folded shading backward's records and clears its accumulator rows; the block is returned as
    the LAST value and goes to shade_backward(..., prepared=), which then launches no setup kernel.

    want_empty_regions=True: a [B, ceil(H/64), ceil(W/64)] uint8 map follows the optional frames (before the
    prepared block): 1 = that 64 x 64 block of the G-buffer holds no candidate triangle (background / transparent
    black); l1_loss_forward(..., empty_a=, empty_b=) and shade_backward(..., empty_regions=) skip such blocks.

    l1_target ([B,H,W,4] float32, contiguous; mr_render_forward_l1): the same pass also compares every pixel it shades
    with the target -- the very LAST value is then (loss, signs), what l1_loss_forward(rgba, l1_target) returns (the
    sum is grouped by region instead of by row: equal to rounding), and no loss kernel has to read the image back.
    l1_target_empty: the target's image_empty_regions map or None; regions empty on both sides are not read.

    private_gbuffer=True (mr_render_forward_l1_private; needs l1_target and prepare_backward, want_z=False): the caller
    keeps the G-buffer to itself and will hand it to shade_backward(..., l1_signs=, prepared=, private_gbuffer=True) only.
    No barycentric plane is written -- `bary` comes back as None -- and `ids` says -1, not 0, where nothing was drawn;
    image, loss, sign codes and the empty-region map have the bits they have without it."""
    if private_gbuffer and (l1_target is None or not prepare_backward or want_z):
        raise ValueError("private_gbuffer needs l1_target and prepare_backward, and leaves no depth plane")
    tensors = [vertices, transforms, normals, diffuse, triangles, light_positions, light_intensities]
    _chk("vertices", vertices, _F32, None, None, 3)
    _chk("triangles", triangles, _I32, None, 3)
    B, V, T = vertices.shape[0], vertices.shape[1], triangles.shape[0]
    _chk("clip-space transforms", transforms, _F32, B, 4, 4)
    for name, t in (("normals", normals), ("diffuse colors", diffuse)):
        _chk(name, t, _F32, B, V, 3)
    _chk_lights(light_positions, light_intensities, ambient, B, shade_max_lights())
    dev = _require_device(*(tensors + ([ambient] if ambient is not None else [])))
    if l1_target is not None:
        _chk("l1_target", l1_target, _F32, B, height, width, 4)
        if l1_target_empty is not None:
            _chk("l1_target_empty", l1_target_empty, _U8, B, (height + 63) // 64, (width + 63) // 64)
        if not l1_target.is_contiguous() or (l1_target_empty is not None and not l1_target_empty.is_contiguous()):
            raise ValueError("l1_target and its map must be contiguous")
        _require_device(vertices, l1_target, *([l1_target_empty] if l1_target_empty is not None else []))
    L = lib()
    vertices, transforms, normals, diffuse, triangles, light_positions, light_intensities = [
        t.contiguous() for t in tensors]
    ambient = ambient.contiguous() if ambient is not None else None
    nl = light_positions.shape[1]
    clip = torch.empty(B, V, 4, dtype=torch.float32, device=dev)
    ids = torch.empty(B, height, width, dtype=torch.int32, device=dev)
    bary = None if private_gbuffer else torch.empty(B, height, width, 3, dtype=torch.float32, device=dev)
    z = torch.empty(B, height, width, dtype=torch.float32, device=dev)
    rgba = torch.empty(B, height, width, 4, dtype=torch.float32, device=dev)
    frames = torch.empty(B, height, width, 4, dtype=torch.uint8, device=dev) if want_u8 else None
    with torch.cuda.device(dev):
        records = _aligned_bytes(L.mr_shade_forward_workspace_bytes(B, V, T, width, height), dev)
        if private_gbuffer:
            prepared = _aligned_bytes(L.mr_render_forward_l1_private_bytes(B, T, width, height), dev)
        else:
            prepared = _aligned_bytes(L.mr_shade_backward_prepared_bytes(B, T), dev) if prepare_backward else None
        empty = (torch.empty(B, (height + 63) // 64, (width + 63) // 64, dtype=torch.uint8, device=dev)
                 if want_empty_regions else None)
        need = L.mr_rasterize_forward_workspace_bytes(B, V, T, width, height)
        ws, have = _workspace(dev, need)
        _arm_timer(TIMER_RASTER_FORWARD)
        args = (_ptr(vertices), _ptr(transforms), _ptr(normals), _ptr(diffuse), _ptr(triangles),
                _ptr(light_positions), _ptr(light_intensities), _ptr(ambient), B, V, T,
                width, height, nl, _ptr(clip), _ptr(ids), _ptr(bary), _ptr(z), int(bool(want_z)),
                _ptr(rgba), _ptr(frames), _ptr(records), _ptr(prepared), _ptr(empty), _ptr(ws), have,
                _stream(dev))
        l1 = None
        if l1_target is None:
            rc = L.mr_render_forward(*args)
        else:
            loss = torch.empty((), dtype=torch.float32, device=dev)
            signs = torch.empty(B * height * width, dtype=torch.uint8, device=dev)
            partials = torch.empty(max(1, L.mr_render_forward_l1_partials(B, width, height)), dtype=torch.float32, device=dev)
            l1_args = (_ptr(l1_target), _ptr(l1_target_empty), _ptr(loss), _ptr(signs), _ptr(partials))
            if private_gbuffer:   # (no `bary`, no `want_z`)
                rc = L.mr_render_forward_l1_private(*(args[:16] + (args[17],) + args[19:] + l1_args))
            else:
                rc = L.mr_render_forward_l1(*args, *l1_args)
            l1 = (loss, signs)
    _check(rc, "mr_render_forward")
    out = (clip, ids, bary, (z if want_z else None), rgba, records) + ((frames,) if want_u8 else ())
    out = out + ((empty,) if want_empty_regions else ()) + ((prepared,) if prepare_backward else ())
    return out + ((l1,) if l1 is not None else ())


def interpolate_raster_max_attributes():
    return int(lib().mr_interpolate_raster_max_attributes())


def interpolate_forward_records(ids, bary, attrs, triangles, background):
    """interpolate_forward through per-(image, triangle) corner records, for at most
    interpolate_raster_max_attributes() attributes -> (out [B,H,W,A], records for the backward)."""
    _chk("triangles", triangles, _I32, None, 3)
    _chk("attributes", attrs, _F32, None, None, None)
    _chk_gbuffer(ids, bary, attrs.shape[0])
    _chk("background", background, _F32, attrs.shape[2])
    if not 1 <= attrs.shape[2] <= interpolate_raster_max_attributes():
        raise ValueError("1..%d attributes are supported here" % interpolate_raster_max_attributes())
    dev = _require_device(ids, bary, attrs, triangles, background)
    L = lib()
    ids, bary, attrs = ids.contiguous(), bary.contiguous(), attrs.contiguous()
    triangles, background = triangles.contiguous(), background.contiguous()
    B, H, W = ids.shape
    V, A, T = attrs.shape[1], attrs.shape[2], triangles.shape[0]
    out = torch.empty(B, H, W, A, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        need = L.mr_interpolate_records_bytes(B, T, A)
        records = _aligned_bytes(need, dev)
        rc = L.mr_interpolate_forward_records(_ptr(ids), _ptr(bary), _ptr(attrs), _ptr(triangles),
                                              _ptr(background), B, V, T, W, H, A, _ptr(out), _ptr(records),
                                              need, _stream(dev))
    _check(rc, "mr_interpolate_forward_records")
    return out, records


def rasterize_interpolate_forward(clip, attrs, triangles, background, width, height):
    """rasterize_clip_space()'s forward in one pass over the pixels (the interpolation is the epilogue of the
    rasterizer's tile walk) for at most interpolate_raster_max_attributes() attributes
    -> (ids [B,H,W], bary [B,H,W,3], out [B,H,W,A], records for interpolate_raster_backward)."""
    B, V, T = _chk_mesh(clip, triangles)
    _chk("attributes", attrs, _F32, B, V, None)
    A = attrs.shape[2]
    _chk("background", background, _F32, A)
    if not 1 <= A <= interpolate_raster_max_attributes():
        raise ValueError("1..%d attributes are supported here" % interpolate_raster_max_attributes())
    dev = _require_device(clip, attrs, triangles, background)
    L = lib()
    clip, attrs, triangles, background = [t.contiguous() for t in (clip, attrs, triangles, background)]
    ids = torch.empty(B, height, width, dtype=torch.int32, device=dev)
    bary = torch.empty(B, height, width, 3, dtype=torch.float32, device=dev)
    z = torch.empty(B, height, width, dtype=torch.float32, device=dev)
    out = torch.empty(B, height, width, A, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        need_rec = L.mr_interpolate_records_bytes(B, T, A)
        records = _aligned_bytes(need_rec, dev)
        need = L.mr_rasterize_forward_workspace_bytes(B, V, T, width, height)
        ws, have = _workspace(dev, need)
        rc = L.mr_rasterize_interpolate_forward(_ptr(clip), _ptr(attrs), _ptr(triangles), _ptr(background), B, V, T,
                                                width, height, A, _ptr(ids), _ptr(bary), _ptr(z), _ptr(out),
                                                _ptr(records), need_rec, _ptr(ws), have, _stream(dev))
    _check(rc, "mr_rasterize_interpolate_forward")
    return ids, bary, out, records


def interpolate_raster_backward(dout, ids, bary, clip, attrs, triangles, background, adjacency,
                                corner_records=None, normalised_gbuffer=False):
    """One-pass backward of interpolation + rasterization -> (dattributes [B,V,A], dclip [B,V,4])."""
    tensors = [dout, ids, bary, clip, attrs, triangles, background, adjacency[0], adjacency[1]]
    B, V, _ = _chk_mesh(clip, triangles)
    _chk("attributes", attrs, _F32, B, V, None)
    h, w = _chk_gbuffer(ids, bary, B)
    _chk("background", background, _F32, attrs.shape[2])
    _chk("upstream gradient", dout, _F32, B, h, w, attrs.shape[2])
    _chk("adjacency offsets", adjacency[0], _I32, V + 1)
    _chk("adjacency entries", adjacency[1], _I32, None)
    dev = _require_device(*tensors)
    L = lib()
    dout, ids, bary, clip, attrs, triangles, background, offsets, entries = [t.contiguous() for t in tensors]
    B, H, W = ids.shape
    V, A, T = attrs.shape[1], attrs.shape[2], triangles.shape[0]
    dattrs = torch.empty(B, V, A, dtype=torch.float32, device=dev)
    dclip = torch.empty(B, V, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _sync_deterministic()
        L.mr_debug_set_shade_backward_kernel(_shade_backward_kernel)
        need = L.mr_interpolate_raster_backward_workspace_bytes(B, V, T, W, H, A)
        ws, have = _workspace(dev, need)
        rc = L.mr_interpolate_raster_backward(
            _ptr(dout), _ptr(ids), _ptr(bary), _ptr(clip), _ptr(attrs), _ptr(triangles), _ptr(background),
            _ptr(offsets), _ptr(entries), _ptr(corner_records), B, V, T, W, H, A, _ptr(dattrs), _ptr(dclip),
            GBUFFER_NORMALISED if normalised_gbuffer else 0, _ptr(ws), have, _stream(dev))
    _check(rc, "mr_interpolate_raster_backward")
    return dattrs, dclip


def vertex_adjacency(triangles, vertex_count):
    """CSR vertex -> (triangle, corner) adjacency of an int32 [T,3] triangle array on its device:
    (offsets [V+1] i32, entries [n] i32), entry = 3 * triangle + corner grouped by vertex; corners
    whose vertex index is out of range are left out.  Cached on the tensor object (keyed by its
    version counter), so a mesh's topology is analysed once."""
    cached = getattr(triangles, "_mr_adjacency", None)
    if cached is not None and cached[0] == (triangles._version, int(vertex_count), triangles.data_ptr()):
        return cached[1], cached[2]
    flat = triangles.reshape(-1).to(torch.int64)
    key = torch.where((flat >= 0) & (flat < vertex_count), flat, torch.full_like(flat, vertex_count))
    order = torch.argsort(key, stable=True)
    # scatter_add, not bincount: bincount reads the maximum back to the host (a device sync on every
    # cache miss, e.g. when the caller passes a fresh `triangles.to(device)` each step)
    counts = torch.zeros(vertex_count + 1, dtype=torch.int64, device=triangles.device)
    counts.scatter_add_(0, key, torch.ones_like(key))
    offsets = torch.zeros(vertex_count + 1, dtype=torch.int64, device=triangles.device)
    offsets[1:] = torch.cumsum(counts[:vertex_count], 0)
    offsets, entries = offsets.to(torch.int32), order.to(torch.int32).contiguous()
    try:
        triangles._mr_adjacency = ((triangles._version, int(vertex_count), triangles.data_ptr()), offsets, entries)
    except AttributeError:
        pass
    return offsets, entries


def antialias_topology(triangles, vertex_count):
    """opposite [T,3] i32 on the triangles' device: for the edge opposite corner k of triangle t, the vertex
    of the neighbouring triangle across it that is not on the edge; -1 for a boundary edge (no neighbour),
    -2 for a non-manifold edge (three or more triangles share it) or a degenerate one (its two vertices are
    the same, or the neighbour repeats a vertex of the edge).  Edges are matched by their unordered vertex
    pair, so winding does not matter.  Torch ops (sort + match): no hot path, and it runs on the CPU too.
    Cached on the tensor object like vertex_adjacency."""
    cached = getattr(triangles, "_mr_aa_opposite", None)
    key = (triangles._version, int(vertex_count), triangles.data_ptr())
    if cached is not None and cached[0] == key:
        return cached[1]
    dev = triangles.device
    tris = triangles.to(torch.int64).reshape(-1, 3)
    T = tris.shape[0]
    # edge k of triangle t joins corners k+1 and k+2; one row per (triangle, edge)
    a = tris[:, [1, 2, 0]].reshape(-1)
    b = tris[:, [2, 0, 1]].reshape(-1)
    c = tris.reshape(-1)                      # the corner opposite the edge
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    n = 3 * T
    opposite = torch.full((n,), -1, dtype=torch.int64, device=dev)
    if n > 0:
        span = int(vertex_count) + 1
        ekey = lo * span + hi
        order = torch.argsort(ekey, stable=True)
        sk = ekey[order]
        new_run = torch.ones(n, dtype=torch.bool, device=dev)
        new_run[1:] = sk[1:] != sk[:-1]
        run = torch.cumsum(new_run.to(torch.int64), 0) - 1
        run_size = torch.zeros(n, dtype=torch.int64, device=dev).scatter_add_(0, run, torch.ones_like(run))
        size = run_size[run]                  # triangles sharing this row's edge (this one included)
        # a run of two: the partner is the other row of the run
        first = torch.zeros(n, dtype=torch.int64, device=dev).scatter_reduce_(
            0, run, torch.arange(n, device=dev), reduce="amin", include_self=False)[run]
        pos = torch.arange(n, device=dev)
        partner = torch.where(pos == first, pos + 1, first).clamp(max=n - 1)
        mate = order[partner]                 # (triangle, edge) row of the neighbour
        d = c[mate]
        sorted_opp = torch.where(size == 2, d, torch.full_like(d, -1))
        sorted_opp = torch.where(size > 2, torch.full_like(d, -2), sorted_opp)
        # degenerate: an edge with one vertex twice, or a neighbour whose far vertex lies on the edge
        degenerate = (lo[order] == hi[order]) | ((size == 2) & ((d == lo[order]) | (d == hi[order])))
        sorted_opp = torch.where(degenerate, torch.full_like(d, -2), sorted_opp)
        opposite[order] = sorted_opp
    opposite = opposite.reshape(T, 3).to(torch.int32).contiguous()
    try:
        triangles._mr_aa_opposite = (key, opposite)
    except AttributeError:
        pass
    return opposite


class MeshTopology:
    """What the mesh regularisers need of a triangle array (mesh_topology()): int32 tensors on the triangles'
    device and the three counts as Python ints.
      edges [E,2]          unique undirected edges (lo, hi), lo < hi, ascending
      nbr_offsets [V+1], nbr [2E]      CSR of every vertex's neighbours, ascending
      flaps [F,4]          (a, b, c, d) per edge that exactly two (triangle, edge) rows share, in the edges' order
      role_offsets [V+1], roles [4F]   CSR of every vertex's flap roles, entry = 4 * flap + role (0..3 = a..d)"""
    __slots__ = ("vertex_count", "edge_count", "flap_count", "edges", "nbr_offsets", "nbr", "flaps", "role_offsets",
                 "roles")

    def __init__(self, vertex_count, edges, nbr_offsets, nbr, flaps, role_offsets, roles):
        self.vertex_count, self.edge_count, self.flap_count = int(vertex_count), edges.shape[0], flaps.shape[0]
        self.edges, self.nbr_offsets, self.nbr = edges, nbr_offsets, nbr
        self.flaps, self.role_offsets, self.roles = flaps, role_offsets, roles

    def tensors(self):
        return (self.edges, self.nbr_offsets, self.nbr, self.flaps, self.role_offsets, self.roles)


def _csr_by_vertex(owner, vertex_count):
    """owner [n] i64 (a vertex per entry) -> (offsets [V+1] i32, order [n] i64): the entries grouped by vertex,
    each group in the entries' own order."""
    order = torch.argsort(owner, stable=True)
    counts = torch.zeros(vertex_count, dtype=torch.int64, device=owner.device)
    counts.scatter_add_(0, owner, torch.ones_like(owner))
    offsets = torch.zeros(vertex_count + 1, dtype=torch.int64, device=owner.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets.to(torch.int32), order


def mesh_topology(triangles, vertex_count):
    """MeshTopology of a [T,3] triangle array of any integer dtype, on its device ("Mesh
    regularisers").  A triangle with an index outside [0, V) is dropped whole, as k_vertex_normals drops it.
    Edges are the unordered vertex pairs of the remaining triangles' sides (a side whose two indices are equal is
    no edge); an edge that exactly two (triangle, side) rows share gives a flap (a, b, c, d) with c the opposite
    corner of the earlier row, unless c or d is a or b (a triangle that repeats an index).  Boundary and
    non-manifold edges give none.  Torch ops (sort + unique): no hot path, it runs on the CPU too, and it reads
    the counts back to the host -- build it before a graph capture.  Cached on the tensor object like
    vertex_adjacency."""
    vertex_count = int(vertex_count)
    key = (triangles._version, vertex_count, triangles.data_ptr())
    cached = getattr(triangles, "_mr_mesh_topology", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    dev = triangles.device
    V = vertex_count
    tris = triangles.to(torch.int64).reshape(-1, 3)
    tris = tris[((tris >= 0) & (tris < V)).all(dim=1)]
    # side k of a triangle joins corners k+1 and k+2 and lies opposite corner k; one row per (triangle, side)
    p = tris[:, [1, 2, 0]].reshape(-1)
    q = tris[:, [2, 0, 1]].reshape(-1)
    opp = tris.reshape(-1)
    lo, hi = torch.minimum(p, q), torch.maximum(p, q)
    keep = lo != hi
    lo, hi, opp = lo[keep], hi[keep], opp[keep]
    ekey = lo * max(V, 1) + hi
    order = torch.argsort(ekey, stable=True)
    sorted_key, sorted_opp = ekey[order], opp[order]
    unique_key, counts = torch.unique_consecutive(sorted_key, return_counts=True)
    edges = torch.stack([unique_key // max(V, 1), unique_key % max(V, 1)], dim=1)
    first = torch.cumsum(counts, 0) - counts
    pair = counts == 2
    a, b = edges[pair, 0], edges[pair, 1]
    c, d = sorted_opp[first[pair]], sorted_opp[(first[pair] + 1).clamp(max=max(sorted_opp.shape[0] - 1, 0))]
    proper = (c != a) & (c != b) & (d != a) & (d != b)
    flaps = torch.stack([a, b, c, d], dim=1)[proper]
    src = torch.cat([edges[:, 0], edges[:, 1]])
    dst = torch.cat([edges[:, 1], edges[:, 0]])
    by_pair = torch.argsort(src * max(V, 1) + dst)
    nbr_offsets, _ = _csr_by_vertex(src, V)
    nbr = dst[by_pair]
    role_offsets, roles = _csr_by_vertex(flaps.reshape(-1), V)
    i32 = lambda t: t.to(torch.int32).contiguous()
    topology = MeshTopology(V, i32(edges), nbr_offsets, i32(nbr), i32(flaps), role_offsets, i32(roles))
    try:
        triangles._mr_mesh_topology = (key, topology)
    except AttributeError:
        pass
    return topology


MESH_LAPLACIAN, MESH_EDGE, MESH_NORMAL = 1, 2, 4   # mesh_raster.h, MR_MESH_*


def _chk_mesh_reg(vertices, topology, terms):
    _chk("vertices", vertices, _F32, None, None, 3)
    B, V, _ = vertices.shape
    if not isinstance(topology, MeshTopology) or topology.vertex_count != V:
        raise ValueError("topology must be the mesh_topology() of the triangles and of these %d vertices" % V)
    if not 0 <= int(terms) <= 7:
        raise ValueError("terms must be a mask of MESH_LAPLACIAN | MESH_EDGE | MESH_NORMAL, got %r" % (terms,))
    if not 1 <= B <= 65535 or V < 1:
        raise ValueError("the mesh regularisers take 1..65535 images of at least one vertex, got %s"
                         % list(vertices.shape))
    E, F = topology.edge_count, topology.flap_count
    _chk("neighbour offsets", topology.nbr_offsets, _I32, V + 1)
    _chk("neighbours", topology.nbr, _I32, 2 * E)
    _chk("flaps", topology.flaps, _I32, F, 4)
    _chk("flap role offsets", topology.role_offsets, _I32, V + 1)
    _chk("flap roles", topology.roles, _I32, 4 * F)
    return B, V, E, F


def mesh_regularizer_forward(vertices, topology, terms, target_length=None):
    """vertices [B,V,3] f32, topology: mesh_topology() -> (terms [B,3] = (lap, edge, nc), unit_dirs [B,V,3] or None
    without MESH_LAPLACIAN).  A term outside the mask `terms` is not computed and reads 0."""
    B, V, E, F = _chk_mesh_reg(vertices, topology, terms)
    dev = _require_device(vertices, *topology.tensors())
    L = lib()
    vertices = vertices.contiguous()
    out = torch.empty(B, 3, dtype=_F32, device=dev)
    unit_dirs = torch.empty(B, V, 3, dtype=_F32, device=dev) if terms & MESH_LAPLACIAN else None
    with torch.cuda.device(dev):
        ws, have = _workspace(dev, L.mr_mesh_regularizer_workspace_bytes(B, V, F)) if terms else (None, 0)
        rc = L.mr_mesh_regularizer_forward(
            _ptr(vertices), _ptr(topology.nbr_offsets), _ptr(topology.nbr), _ptr(topology.flaps), B, V, E, F,
            int(terms), 0 if target_length is None else 1, 0.0 if target_length is None else float(target_length),
            _ptr(unit_dirs), _ptr(out), _ptr(ws), have, _stream(dev))
    _check(rc, "mr_mesh_regularizer_forward")
    return out, unit_dirs


def mesh_regularizer_backward(dterms, vertices, unit_dirs, topology, terms, target_length=None):
    """dterms [B,3] f32 (device) -> dvertices [B,V,3]; unit_dirs as the forward returned them."""
    B, V, E, F = _chk_mesh_reg(vertices, topology, terms)
    _chk("upstream gradient", dterms, _F32, B, 3)
    if terms & MESH_LAPLACIAN:
        _chk("unit directions", unit_dirs, _F32, B, V, 3)
    tensors = [dterms, vertices] + ([unit_dirs] if terms & MESH_LAPLACIAN else []) + list(topology.tensors())
    dev = _require_device(*tensors)
    L = lib()
    dterms, vertices = dterms.contiguous(), vertices.contiguous()
    unit_dirs = unit_dirs.contiguous() if terms & MESH_LAPLACIAN else None
    dvertices = torch.empty(B, V, 3, dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        rc = L.mr_mesh_regularizer_backward(
            _ptr(dterms), _ptr(vertices), _ptr(unit_dirs), _ptr(topology.nbr_offsets), _ptr(topology.nbr),
            _ptr(topology.flaps), _ptr(topology.role_offsets), _ptr(topology.roles), B, V, E, F, int(terms),
            0 if target_length is None else 1, 0.0 if target_length is None else float(target_length),
            _ptr(dvertices), _stream(dev))
    _check(rc, "mr_mesh_regularizer_backward")
    return dvertices


def _plan(name, args, fields, takes):
    """One mr_*_plan call: the native function `name` over the int `args`, its outputs under `fields`; it refuses
    what the matching forward refuses, `takes` says what that is."""
    out = (ctypes.c_int * len(fields))()
    rc = getattr(lib(), "mr_" + name)(*[int(a) for a in args],
                                      *[ctypes.c_void_p(ctypes.addressof(out) + 4 * k) for k in range(len(fields))])
    if rc != MR_OK:
        raise ValueError("%s takes %s, got (%s)" % (name, takes, ", ".join("%r" % (a,) for a in args)))
    return dict(zip(fields, list(out)))


def nearest_plan(B, N, M):
    """The launch shape mr_nearest_forward takes for B images of N queries against M targets, a pure host function:
    {"splits", "queries_per_lane", "target_tile", "workgroup_size"} (include/mesh_raster.h)."""
    return _plan("nearest_plan", (B, N, M), ("splits", "queries_per_lane", "target_tile", "workgroup_size"),
                 "1..65535 images of 1..2^28 points")


def _chk_clouds(x, y, x_lengths, y_lengths):
    _chk("x", x, _F32, None, None, 3)
    B, N, _ = x.shape
    _chk("y", y, _F32, B, None, 3)
    M = y.shape[1]
    if not 1 <= B <= 65535 or not 1 <= N <= 1 << 28 or not 1 <= M <= 1 << 28 or B * N >= 1 << 36 or B * M >= 1 << 36:
        raise ValueError("the point-cloud kernels take 1..65535 images of 1..2^28 points, got %s and %s"
                         % (list(x.shape), list(y.shape)))
    for name, t in (("x_lengths", x_lengths), ("y_lengths", y_lengths)):
        if t is not None:
            _chk(name, t, _I32, B)
    return B, N, M


def nearest_forward(x, y, x_lengths=None, y_lengths=None, want_sqdist=True, total=None, weight=1.0):
    """x [B,N,3], y [B,M,3] f32, lengths [B] i32 or None (device) -> (sqdist [B,N] f32 or None, idx [B,N] i32,
    total [B] f32 or None): mr_nearest_forward.  total: None = no mean; True = a fresh [B] tensor set to weight *
    mean; a [B] tensor = weight * mean is added to it (Chamfer's second direction)."""
    B, N, M = _chk_clouds(x, y, x_lengths, y_lengths)
    given = [t for t in (x_lengths, y_lengths) if t is not None]
    accumulate = torch.is_tensor(total)
    if accumulate:
        _chk("total", total, _F32, B)
        if not total.is_contiguous():
            raise ValueError("total must be contiguous")
        given.append(total)
    dev = _require_device(x, y, *given)
    L = lib()
    x, y = x.contiguous(), y.contiguous()
    x_lengths = x_lengths.contiguous() if x_lengths is not None else None
    y_lengths = y_lengths.contiguous() if y_lengths is not None else None
    sqdist = torch.empty(B, N, dtype=_F32, device=dev) if want_sqdist else None
    idx = torch.empty(B, N, dtype=_I32, device=dev)
    if total is True:
        total = torch.empty(B, dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        ws, have = _workspace(dev, L.mr_nearest_workspace_bytes(B, N, M))
        rc = L.mr_nearest_forward(_ptr(x), _ptr(y), _ptr(x_lengths), _ptr(y_lengths), B, N, M, _ptr(sqdist), _ptr(idx),
                                  _ptr(total), float(weight), 1 if accumulate else 0, _ptr(ws), have, _stream(dev))
    _check(rc, "mr_nearest_forward")
    return sqdist, idx, total


def nearest_inverted_index(idx, targets):
    """idx [B,Q] i32 (-1 = no neighbour) into `targets` points -> (order [B,Q] i32, offsets [B,targets+1] i32): per
    image the queries grouped by the target they chose, each group in ascending query order (a STABLE sort, so the
    backward's sums have a fixed order), group j at order[b, offsets[b,j]:offsets[b,j+1]]; queries without a neighbour
    come after offsets[b,targets].  Device-side torch ops (sort + searchsorted), no host synchronisation."""
    _chk("idx", idx, _I32, None, None)
    key = torch.where(idx < 0, torch.full_like(idx, targets), idx)
    sorted_key, order = torch.sort(key, dim=1, stable=True)
    bounds = torch.arange(targets + 1, dtype=_I32, device=idx.device).unsqueeze(0).expand(idx.shape[0], -1).contiguous()
    offsets = torch.searchsorted(sorted_key, bounds, out_int32=True)
    return order.to(_I32), offsets


def nearest_backward(x, y, x_lengths, y_lengths, idx_xy=None, index_xy=None, idx_yx=None, index_yx=None,
                     grad_points=None, grad_images=None, x_weight=1.0, y_weight=1.0, want_dx=True, want_dy=True):
    """mr_nearest_backward -> (dx [B,N,3] or None, dy [B,M,3] or None).  idx_xy / idx_yx: the saved indices of the
    directions that ran; index_xy / index_yx: their nearest_inverted_index(), needed for dy / dx respectively."""
    B, N, M = _chk_clouds(x, y, x_lengths, y_lengths)
    tensors = [x, y] + [t for t in (x_lengths, y_lengths) if t is not None]
    for name, idx, index, Q, T in (("xy", idx_xy, index_xy, N, M), ("yx", idx_yx, index_yx, M, N)):
        if idx is not None:
            _chk("idx_" + name, idx, _I32, B, Q)
            tensors.append(idx)
        if index is not None:
            _chk("order_" + name, index[0], _I32, B, Q)
            _chk("offsets_" + name, index[1], _I32, B, T + 1)
            tensors += list(index)
    if grad_points is not None:
        _chk("upstream gradient", grad_points, _F32, B, N)
        tensors.append(grad_points)
    if grad_images is not None:
        _chk("upstream gradient", grad_images, _F32, B)
        tensors.append(grad_images)
    dev = _require_device(*tensors)
    L = lib()
    c = lambda t: t.contiguous() if t is not None else None
    order_xy, offsets_xy = index_xy if index_xy is not None else (None, None)
    order_yx, offsets_yx = index_yx if index_yx is not None else (None, None)
    dx = torch.empty(B, N, 3, dtype=_F32, device=dev) if want_dx else None
    dy = torch.empty(B, M, 3, dtype=_F32, device=dev) if want_dy else None
    held = [c(t) for t in (x, y, x_lengths, y_lengths, idx_xy, order_xy, offsets_xy, idx_yx, order_yx, offsets_yx,
                           grad_points, grad_images)]
    with torch.cuda.device(dev):
        rc = L.mr_nearest_backward(*[_ptr(t) for t in held[:4]], B, N, M, *[_ptr(t) for t in held[4:]],
                                   float(x_weight), float(y_weight), _ptr(dx), _ptr(dy), _stream(dev))
    _check(rc, "mr_nearest_backward")
    return dx, dy


KNN_MAX_K = 32


def knn_plan(B, N, M, K):
    """The launch shape mr_knn_forward takes for B images of N queries against M targets and K neighbours, a pure
    host function: {"splits", "queries_per_lane", "list_capacity", "target_tile", "workgroup_size"}
    (include/mesh_raster.h)."""
    return _plan("knn_plan", (B, N, M, K),
                 ("splits", "queries_per_lane", "list_capacity", "target_tile", "workgroup_size"),
                 "1..65535 images of 1..2^28 points and 1..%d neighbours with N * K < 2^31" % KNN_MAX_K)


def _chk_knn(x, y, x_lengths, y_lengths, K):
    B, N, M = _chk_clouds(x, y, x_lengths, y_lengths)
    if not isinstance(K, int) or isinstance(K, bool) or not 1 <= K <= KNN_MAX_K:
        raise ValueError("K must be an int in [1, %d], got %r" % (KNN_MAX_K, K))
    if N * K >= 1 << 31 or B * N * K >= 1 << 36:
        raise ValueError("the K-nearest-neighbour kernels take N * K < 2^31 and B * N * K < 2^36, got %s with K = %d"
                         % (list(x.shape), K))
    return B, N, M


def knn_forward(x, y, K, x_lengths=None, y_lengths=None):
    """x [B,N,3], y [B,M,3] f32, lengths [B] i32 or None (device) -> (sqdist [B,N,K] f32, idx [B,N,K] i32):
    mr_knn_forward."""
    B, N, M = _chk_knn(x, y, x_lengths, y_lengths, K)
    dev = _require_device(x, y, *[t for t in (x_lengths, y_lengths) if t is not None])
    L = lib()
    x, y = x.contiguous(), y.contiguous()
    x_lengths = x_lengths.contiguous() if x_lengths is not None else None
    y_lengths = y_lengths.contiguous() if y_lengths is not None else None
    sqdist = torch.empty(B, N, K, dtype=_F32, device=dev)
    idx = torch.empty(B, N, K, dtype=_I32, device=dev)
    with torch.cuda.device(dev):
        ws, have = _workspace(dev, L.mr_knn_workspace_bytes(B, N, M, K))
        rc = L.mr_knn_forward(_ptr(x), _ptr(y), _ptr(x_lengths), _ptr(y_lengths), B, N, M, K, _ptr(sqdist), _ptr(idx),
                              _ptr(ws), have, _stream(dev))
    _check(rc, "mr_knn_forward")
    return sqdist, idx


def knn_backward(x, y, x_lengths, y_lengths, sqdist, idx, grad, index=None, want_dx=True, want_dy=True):
    """mr_knn_backward -> (dx [B,N,3] or None, dy [B,M,3] or None).  sqdist, idx [B,N,K]: what knn_forward returned;
    grad [B,N,K] f32; index: nearest_inverted_index(idx.reshape(B, N * K), M), needed for dy."""
    _chk("idx", idx, _I32, None, None, None)
    K = int(idx.shape[2])
    B, N, M = _chk_knn(x, y, x_lengths, y_lengths, K)
    _chk("idx", idx, _I32, B, N, K)
    _chk("sqdist", sqdist, _F32, B, N, K)
    _chk("upstream gradient", grad, _F32, B, N, K)
    tensors = [x, y, sqdist, idx, grad] + [t for t in (x_lengths, y_lengths) if t is not None]
    if index is not None:
        _chk("order", index[0], _I32, B, N * K)
        _chk("offsets", index[1], _I32, B, M + 1)
        tensors += list(index)
    elif want_dy:
        raise ValueError("the targets' gradient needs the inverted index of idx")
    dev = _require_device(*tensors)
    L = lib()
    c = lambda t: t.contiguous() if t is not None else None
    order, offsets = index if index is not None else (None, None)
    dx = torch.empty(B, N, 3, dtype=_F32, device=dev) if want_dx else None
    dy = torch.empty(B, M, 3, dtype=_F32, device=dev) if want_dy else None
    held = [c(t) for t in (x, y, x_lengths, y_lengths, sqdist, idx, order, offsets, grad)]
    with torch.cuda.device(dev):
        rc = L.mr_knn_backward(*[_ptr(t) for t in held[:4]], B, N, M, K, *[_ptr(t) for t in held[4:]], _ptr(dx),
                               _ptr(dy), _stream(dev))
    _check(rc, "mr_knn_backward")
    return dx, dy


FARTHEST_ROUTE_PLAN, FARTHEST_ROUTE_RESIDENT, FARTHEST_ROUTE_STEPS = 0, 1, 2   # mr_farthest_forward's `route`
_FARTHEST_TAKES = "1..65535 clouds of 1..2^28 - 1 points and 1..2^24 - 1 samples with B * K < 2^31"


def farthest_plan(B, N, K):
    """The route and launch shape mr_farthest_forward takes for B clouds of N points and K samples, a pure host
    function: {"route" (1: one launch, the cloud in one workgroup's registers; 2: one launch per step),
    "workgroup_size", "points_per_lane", "slices"} (include/mesh_raster.h)."""
    return _plan("farthest_plan", (B, N, K), ("route", "workgroup_size", "points_per_lane", "slices"), _FARTHEST_TAKES)


def debug_set_farthest_shape(workgroup_size, points_per_lane):
    """Measurement and tests (include/mesh_raster_debug.h): route 1's launch shape for THIS thread's next calls;
    (0, 0) = the plan's."""
    _check(lib().mr_debug_set_farthest_shape(int(workgroup_size), int(points_per_lane)), "mr_debug_set_farthest_shape")


def _chk_farthest(points, K, lengths, start_idx):
    _chk("points", points, _F32, None, None, 3)
    B, N, _ = points.shape
    if not isinstance(K, int) or isinstance(K, bool) or not 1 <= K < 1 << 24:
        raise ValueError("K must be an int in [1, 2^24), got %r" % (K,))
    if not 1 <= B <= 65535 or not 1 <= N < 1 << 28 or B * K >= 1 << 31:
        raise ValueError("farthest-point sampling takes %s, got %s with K = %d" % (_FARTHEST_TAKES, list(points.shape), K))
    for name, t in (("lengths", lengths), ("start_idx", start_idx)):
        if t is not None:
            _chk(name, t, _I32, B)
    return B, N


def farthest_forward(points, K, lengths=None, start_idx=None, route=FARTHEST_ROUTE_PLAN):
    """points [B,N,3] f32, lengths / start_idx [B] i32 or None (device) -> (idx [B,K] i32, radius [B,K] f32):
    mr_farthest_forward.  route: FARTHEST_ROUTE_PLAN, or one of the two forced (a forced FARTHEST_ROUTE_RESIDENT
    that cannot hold N is a ValueError)."""
    B, N = _chk_farthest(points, K, lengths, start_idx)
    if route not in (FARTHEST_ROUTE_PLAN, FARTHEST_ROUTE_RESIDENT, FARTHEST_ROUTE_STEPS):
        raise ValueError("route must be 0 (the plan's), 1 or 2, got %r" % (route,))
    dev = _require_device(points, *[t for t in (lengths, start_idx) if t is not None])
    L = lib()
    points = points.contiguous()
    lengths = lengths.contiguous() if lengths is not None else None
    start_idx = start_idx.contiguous() if start_idx is not None else None
    idx = torch.empty(B, K, dtype=_I32, device=dev)
    radius = torch.empty(B, K, dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        ws, have = _workspace(dev, L.mr_farthest_workspace_bytes(B, N, K))
        rc = L.mr_farthest_forward(_ptr(points), _ptr(lengths), _ptr(start_idx), B, N, K, int(route), _ptr(idx),
                                   _ptr(radius), _ptr(ws), have, _stream(dev))
    if rc == MR_EINVAL and route == FARTHEST_ROUTE_RESIDENT:
        raise ValueError("the one-workgroup route of farthest-point sampling cannot hold %d points" % N)
    _check(rc, "mr_farthest_forward")
    return idx, radius


LAPLACIAN_ROUTE_PLAN, LAPLACIAN_ROUTE_RESIDENT, LAPLACIAN_ROUTE_STEPS = 0, 1, 2   # mr_laplacian_solve's `route`
_LAPLACIAN_TAKES = "1..2^28 - 1 vertices and 1..4 channels"


def laplacian_solve_plan(V, C, route=None):
    """The route and launch shape mr_laplacian_solve takes for V vertices and C channels, a pure host function of
    the two: {"route" (1: one launch, the image in one workgroup's registers; 2: two launches per iteration),
    "workgroup_size", "vertices_per_lane"} (include/mesh_raster.h).  route forces one; a forced resident route that
    cannot hold V is a ValueError."""
    plan = _plan("laplacian_solve_plan", (V, C, route or 0), ("route", "workgroup_size", "vertices_per_lane", "slices"),
                 _LAPLACIAN_TAKES + " on a route that holds them")
    del plan["slices"]
    return plan


def _chk_laplacian(x, topology, lam, name="x"):
    _chk(name, x, _F32, None, None, None)
    B, V, C = x.shape
    if not isinstance(topology, MeshTopology) or topology.vertex_count != V:
        raise ValueError("topology must be the mesh_topology() of the triangles and of these %d vertices" % V)
    if not 1 <= B <= 65535 or not 1 <= V < 1 << 28 or not 1 <= C <= 4 or B * V * C >= 1 << 36:
        raise ValueError("the Laplacian solve takes 1..65535 images of %s, got %s" % (_LAPLACIAN_TAKES, list(x.shape)))
    lam = float(lam)
    if not 0.0 <= lam < float("inf"):
        raise ValueError("lam must be a finite number >= 0, got %r" % (lam,))
    _chk("neighbour offsets", topology.nbr_offsets, _I32, V + 1)
    _chk("neighbours", topology.nbr, _I32, 2 * topology.edge_count)
    return B, V, C, lam


def laplacian_apply(x, topology, lam):
    """x [B,V,C] f32 (device), topology: mesh_topology() of these V vertices -> (I + lam L) x: mr_laplacian_apply."""
    B, V, C, lam = _chk_laplacian(x, topology, lam)
    dev = _require_device(x, topology.nbr_offsets, topology.nbr)
    x = x.contiguous()
    y = torch.empty_like(x)
    with torch.cuda.device(dev):
        rc = lib().mr_laplacian_apply(_ptr(x), _ptr(topology.nbr_offsets), _ptr(topology.nbr), B, V, C,
                                      topology.nbr.shape[0], lam, _ptr(y), _stream(dev))
    _check(rc, "mr_laplacian_apply")
    return y


def laplacian_solve(b, topology, lam, tol=1e-6, max_iterations=300, x0=None, check_every=0, route=None):
    """b [B,V,C] f32 (device), x0 the same or None -> (x, iterations [B,C] i32, residual [B,C] f32) with
    (I + lam L) x = b: mr_laplacian_solve.  check_every = 0 enqueues the whole solve and reads nothing back; k > 0
    reads one word every k iterations of the stepped route and stops launching once every system is frozen (the
    resident route leaves its loop by itself).  route: None, or LAPLACIAN_ROUTE_RESIDENT / _STEPS forced (a forced
    resident route that cannot hold V is a ValueError)."""
    B, V, C, lam = _chk_laplacian(b, topology, lam, "b")
    tol, max_iterations, check_every = float(tol), int(max_iterations), int(check_every)
    if not 0.0 <= tol < float("inf"):
        raise ValueError("tol must be a finite number >= 0, got %r" % (tol,))
    if not 0 <= max_iterations <= 10000:
        raise ValueError("max_iterations must lie in 0..10000, got %r" % (max_iterations,))
    if check_every < 0:
        raise ValueError("check_every must be >= 0, got %r" % (check_every,))
    if route not in (None, LAPLACIAN_ROUTE_PLAN, LAPLACIAN_ROUTE_RESIDENT, LAPLACIAN_ROUTE_STEPS):
        raise ValueError("route must be None, 1 (resident) or 2 (stepped), got %r" % (route,))
    if x0 is not None:
        _chk("x0", x0, _F32, B, V, C)
    dev = _require_device(b, topology.nbr_offsets, topology.nbr, *([x0] if x0 is not None else []))
    if check_every and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("check_every > 0 reads back from the device, which a stream capture cannot do: "
                           "capture the solve with check_every=0")
    stepped = laplacian_solve_plan(V, C, route)["route"] == LAPLACIAN_ROUTE_STEPS   # (ValueError: a forced route 1)
    L = lib()
    b = b.contiguous()
    x0 = x0.contiguous() if x0 is not None else None
    x = torch.empty_like(b)
    iterations = torch.empty(B, C, dtype=_I32, device=dev)
    residual = torch.empty(B, C, dtype=_F32, device=dev)
    chunk = check_every if stepped and check_every else max(max_iterations, 1)
    all_frozen = torch.empty(B, dtype=_I32, device=dev) if chunk < max_iterations else None
    with torch.cuda.device(dev):
        ws, have = _workspace(dev, L.mr_laplacian_solve_workspace_bytes(B, V, C))
        stream = _stream(dev)

        def run(first, count):
            _check(L.mr_laplacian_solve(_ptr(b), _ptr(x0), _ptr(topology.nbr_offsets), _ptr(topology.nbr), B, V, C,
                                        topology.nbr.shape[0], lam, tol, max_iterations, int(route or 0), first, count,
                                        _ptr(all_frozen), _ptr(x), _ptr(iterations), _ptr(residual), _ptr(ws), have,
                                        stream), "mr_laplacian_solve")

        first = 0
        while True:
            run(first, chunk)
            first += chunk
            if first >= max_iterations:
                break
            if bool((all_frozen != 0).all()):   # the only read-back of the loop
                run(max_iterations, 0)
                break
    return x, iterations, residual


def _chk_align(x, lengths, weights=None):
    _chk("x", x, _F32, None, None, 3)
    B, N, _ = x.shape
    if not 1 <= B <= 65535 or not 1 <= N <= 1 << 28 or B * N >= 1 << 36:
        raise ValueError("the registration kernels take 1..65535 images of 1..2^28 points, got %s" % list(x.shape))
    if lengths is not None:
        _chk("lengths", lengths, _I32, B)
    if weights is not None:
        _chk("weights", weights, _F32, B, N)
    return B, N


def align_solve(x, y, weights=None, lengths=None, idx=None, gather=False, sqdist=None, max_sqdist=float("inf"),
                estimate_scale=False, allow_reflection=False):
    """x [B,N,3] f32; y [B,N,3] matched row by row, or with gather y [B,M,3] read at idx [B,N] i32 (idx < 0 or >= M:
    the row is dropped; without gather idx only marks rows); weights / sqdist [B,N] f32, lengths [B] i32 or None
    (device) -> (R [B,3,3], T [B,3], s [B], rmse [B]) f32: mr_align_solve without ICP's bookkeeping."""
    B, N = _chk_align(x, lengths, weights)
    _chk("y", y, _F32, B, None if gather else N, 3)
    M = y.shape[1]
    if not 1 <= M <= 1 << 28 or B * M >= 1 << 36:
        raise ValueError("the registration kernels take 1..65535 images of 1..2^28 points, got %s" % list(y.shape))
    if gather and idx is None:
        raise ValueError("gather needs idx")
    for name, t, dtype in (("idx", idx, _I32), ("sqdist", sqdist, _F32)):
        if t is not None:
            _chk(name, t, dtype, B, N)
    given = [t for t in (weights, lengths, idx, sqdist) if t is not None]
    dev = _require_device(x, y, *given)
    L = lib()
    x, y = x.contiguous(), y.contiguous()
    weights, lengths, idx, sqdist = (t.contiguous() if t is not None else None for t in (weights, lengths, idx, sqdist))
    R = torch.empty(B, 3, 3, dtype=_F32, device=dev)
    T = torch.empty(B, 3, dtype=_F32, device=dev)
    s = torch.empty(B, dtype=_F32, device=dev)
    rmse = torch.empty(B, dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        ws, have = _workspace(dev, L.mr_align_workspace_bytes(B, N))
        rc = L.mr_align_solve(_ptr(x), _ptr(y), _ptr(idx), 1 if gather else 0, _ptr(weights), _ptr(sqdist),
                              float(max_sqdist), _ptr(lengths), B, N, M, 1 if estimate_scale else 0,
                              1 if allow_reflection else 0, 0.0, _ptr(R), _ptr(T), _ptr(s), _ptr(rmse), None, None, None,
                              _ptr(ws), have, _stream(dev))
    _check(rc, "mr_align_solve")
    return R, T, s, rmse


def align_apply(x, R, T, s, lengths=None):
    """x [B,N,3], R [B,3,3], T [B,3], s [B] f32, lengths [B] i32 or None (device) -> s x R + T [B,N,3], 0 in padded
    rows: mr_align_apply."""
    B, N = _chk_align(x, lengths)
    _chk("R", R, _F32, B, 3, 3)
    _chk("T", T, _F32, B, 3)
    _chk("s", s, _F32, B)
    dev = _require_device(x, R, T, s, *([lengths] if lengths is not None else []))
    x, R, T, s = x.contiguous(), R.contiguous(), T.contiguous(), s.contiguous()
    lengths = lengths.contiguous() if lengths is not None else None
    xt = torch.empty_like(x)
    with torch.cuda.device(dev):
        rc = lib().mr_align_apply(_ptr(x), _ptr(lengths), _ptr(R), _ptr(T), _ptr(s), B, N, _ptr(xt), _stream(dev))
    _check(rc, "mr_align_apply")
    return xt


def icp(x, y=None, mesh=None, x_lengths=None, y_lengths=None, init=None, max_iterations=100, relative_rmse_thr=1e-6,
        estimate_scale=False, allow_reflection=False, max_sqdist=None, check_every=10):
    """The rounds of iterative_closest_point on the device.  x [B,N,3] f32 against a cloud y [B,M,3] (y_lengths) or a
    mesh = (vertices [B,V,3] f32, triangles [T,3] i32); init = (R, T, s) or None -> (converged [B] i32, rmse [B],
    xt [B,N,3], R, T, s, iterations [B] i32).  A round is mr_align_apply, the search (mr_nearest_forward, or
    mr_nearest_triangle_forward and mr_align_closest_points), mr_align_solve; every buffer is allocated before the
    first round, and nothing is read back unless check_every > 0 (then `converged` every check_every rounds)."""
    B, N = _chk_align(x, x_lengths)
    if (y is None) == (mesh is None):
        raise ValueError("exactly one of y and mesh must be given")
    given = [t for t in (x_lengths, y_lengths) if t is not None]
    if mesh is None:
        B, N, M = _chk_clouds(x, y, x_lengths, y_lengths)
        given.append(y)
    else:
        vertices, triangles = mesh
        B, N, V, Tn = _chk_point_mesh(x, vertices, triangles, x_lengths)
        given += [vertices, triangles]
    if init is not None:
        _chk("init R", init[0], _F32, B, 3, 3)
        _chk("init T", init[1], _F32, B, 3)
        _chk("init s", init[2], _F32, B)
        given += list(init)
    dev = _require_device(x, *given)
    L = lib()
    x = x.contiguous()
    x_lengths = x_lengths.contiguous() if x_lengths is not None else None
    y_lengths = y_lengths.contiguous() if y_lengths is not None else None
    R0, T0, s0 = (t.contiguous() for t in init) if init is not None else (None, None, None)
    R = torch.empty(B, 3, 3, dtype=_F32, device=dev)
    T = torch.empty(B, 3, dtype=_F32, device=dev)
    s = torch.empty(B, dtype=_F32, device=dev)
    rmse = torch.empty(B, dtype=_F32, device=dev)
    converged = torch.empty(B, dtype=_I32, device=dev)
    iterations = torch.empty(B, dtype=_I32, device=dev)
    prev_rmse = torch.empty(B, dtype=torch.float64, device=dev)
    xt = torch.empty_like(x)
    sqdist = torch.empty(B, N, dtype=_F32, device=dev)
    idx = torch.empty(B, N, dtype=_I32, device=dev)
    cut = float(max_sqdist) if max_sqdist is not None else float("inf")
    cut_plane = sqdist if max_sqdist is not None else None
    if mesh is None:
        y = y.contiguous()
        search_bytes = L.mr_nearest_workspace_bytes(B, N, M)
    else:
        vertices, triangles = vertices.contiguous(), triangles.contiguous()
        bary = torch.empty(B, N, 3, dtype=_F32, device=dev)
        closest = torch.empty(B, N, 3, dtype=_F32, device=dev)
        search_bytes = L.mr_nearest_triangle_workspace_bytes(B, N, Tn)
    stream = _stream(dev)
    with torch.cuda.device(dev):
        ws, have = _workspace(dev, max(search_bytes, L.mr_align_workspace_bytes(B, N)))
        _check(L.mr_align_icp_init(_ptr(R0), _ptr(T0), _ptr(s0), B, _ptr(R), _ptr(T), _ptr(s), _ptr(rmse),
                                   _ptr(converged), _ptr(iterations), _ptr(prev_rmse), stream), "mr_align_icp_init")
        for round_ in range(max_iterations):
            _check(L.mr_align_apply(_ptr(x), _ptr(x_lengths), _ptr(R), _ptr(T), _ptr(s), B, N, _ptr(xt), stream),
                   "mr_align_apply")
            if mesh is None:
                _check(L.mr_nearest_forward(_ptr(xt), _ptr(y), _ptr(x_lengths), _ptr(y_lengths), B, N, M, _ptr(sqdist),
                                            _ptr(idx), None, 1.0, 0, _ptr(ws), have, stream), "mr_nearest_forward")
                target, gather, rows = y, 1, M
            else:
                _check(L.mr_nearest_triangle_forward(_ptr(xt), _ptr(vertices), _ptr(triangles), _ptr(x_lengths), B, N, V,
                                                     Tn, _ptr(sqdist), _ptr(idx), _ptr(bary), None, _ptr(ws), have,
                                                     stream), "mr_nearest_triangle_forward")
                _check(L.mr_align_closest_points(_ptr(vertices), _ptr(triangles), _ptr(idx), _ptr(bary), B, N, V, Tn,
                                                 _ptr(closest), stream), "mr_align_closest_points")
                target, gather, rows = closest, 0, N
            _check(L.mr_align_solve(_ptr(x), _ptr(target), _ptr(idx), gather, None, _ptr(cut_plane), cut,
                                    _ptr(x_lengths), B, N, rows, 1 if estimate_scale else 0,
                                    1 if allow_reflection else 0, float(relative_rmse_thr), _ptr(R), _ptr(T), _ptr(s),
                                    _ptr(rmse), _ptr(converged), _ptr(iterations), _ptr(prev_rmse), _ptr(ws), have,
                                    stream), "mr_align_solve")
            if check_every and (round_ + 1) % check_every == 0 and round_ + 1 < max_iterations:
                if bool((converged != 0).all()):   # the only read-back of the loop
                    break
        _check(L.mr_align_apply(_ptr(x), _ptr(x_lengths), _ptr(R), _ptr(T), _ptr(s), B, N, _ptr(xt), stream),
               "mr_align_apply")
    return converged, rmse, xt, R, T, s, iterations


def nearest_triangle_plan(B, N, T):
    """The launch shape mr_nearest_triangle_forward takes for B images of N queries against T triangles, a pure host
    function: {"splits", "queries_per_lane", "triangle_tile", "workgroup_size"} (include/mesh_raster.h)."""
    return _plan("nearest_triangle_plan", (B, N, T),
                 ("splits", "queries_per_lane", "triangle_tile", "workgroup_size"),
                 "1..65535 images of 1..2^28 points and triangles")


def _chk_point_mesh(points, vertices, triangles, lengths):
    _chk("points", points, _F32, None, None, 3)
    B, N, _ = points.shape
    _chk("vertices", vertices, _F32, B, None, 3)
    V = vertices.shape[1]
    _chk("triangles", triangles, _I32, None, 3)
    T = triangles.shape[0]
    if (not 1 <= B <= 65535 or not all(1 <= n <= 1 << 28 and B * n < 1 << 36 for n in (N, V, T))):
        raise ValueError("the point-to-mesh kernels take 1..65535 images of 1..2^28 points, vertices and triangles, "
                         "got %s, %s and %s" % (list(points.shape), list(vertices.shape), list(triangles.shape)))
    if lengths is not None:
        _chk("lengths", lengths, _I32, B)
    return B, N, V, T


def nearest_triangle_forward(points, vertices, triangles, lengths=None, want_sqdist=True, want_total=False):
    """points [B,N,3], vertices [B,V,3] f32, triangles [T,3] i32, lengths [B] i32 or None (device) -> (sqdist [B,N]
    f32 or None, face [B,N] i32, bary [B,N,3] f32, total [B] f32 or None: the mean of sqdist over each image's valid
    queries): mr_nearest_triangle_forward."""
    B, N, V, T = _chk_point_mesh(points, vertices, triangles, lengths)
    dev = _require_device(points, vertices, triangles, *([lengths] if lengths is not None else []))
    L = lib()
    points, vertices, triangles = points.contiguous(), vertices.contiguous(), triangles.contiguous()
    lengths = lengths.contiguous() if lengths is not None else None
    sqdist = torch.empty(B, N, dtype=_F32, device=dev) if want_sqdist else None
    face = torch.empty(B, N, dtype=_I32, device=dev)
    bary = torch.empty(B, N, 3, dtype=_F32, device=dev)
    total = torch.empty(B, dtype=_F32, device=dev) if want_total else None
    with torch.cuda.device(dev):
        ws, have = _workspace(dev, L.mr_nearest_triangle_workspace_bytes(B, N, T))
        rc = L.mr_nearest_triangle_forward(_ptr(points), _ptr(vertices), _ptr(triangles), _ptr(lengths), B, N, V, T,
                                           _ptr(sqdist), _ptr(face), _ptr(bary), _ptr(total), _ptr(ws), have,
                                           _stream(dev))
    _check(rc, "mr_nearest_triangle_forward")
    return sqdist, face, bary, total


def nearest_triangle_backward(points, vertices, triangles, lengths, face, bary, index=None, grad_points=None,
                              grad_images=None, want_dpoints=True, want_dvertices=True):
    """mr_nearest_triangle_backward -> (dpoints [B,N,3] or None, dvertices [B,V,3] or None).  index: (order [B,3N],
    offsets [B,V+1]), nearest_inverted_index() of the (query, corner) entries' vertices, needed for dvertices."""
    B, N, V, T = _chk_point_mesh(points, vertices, triangles, lengths)
    _chk("face", face, _I32, B, N)
    _chk("bary", bary, _F32, B, N, 3)
    tensors = [points, vertices, triangles, face, bary] + ([lengths] if lengths is not None else [])
    if index is not None:
        _chk("order", index[0], _I32, B, 3 * N)
        _chk("offsets", index[1], _I32, B, V + 1)
        tensors += list(index)
    if grad_points is not None:
        _chk("upstream gradient", grad_points, _F32, B, N)
        tensors.append(grad_points)
    if grad_images is not None:
        _chk("upstream gradient", grad_images, _F32, B)
        tensors.append(grad_images)
    dev = _require_device(*tensors)
    L = lib()
    c = lambda t: t.contiguous() if t is not None else None
    order, offsets = index if index is not None else (None, None)
    dpoints = torch.empty(B, N, 3, dtype=_F32, device=dev) if want_dpoints else None
    dvertices = torch.empty(B, V, 3, dtype=_F32, device=dev) if want_dvertices else None
    held = [c(t) for t in (points, vertices, triangles, lengths, face, bary, order, offsets, grad_points, grad_images)]
    with torch.cuda.device(dev):
        rc = L.mr_nearest_triangle_backward(*[_ptr(t) for t in held[:4]], B, N, V, T, *[_ptr(t) for t in held[4:]],
                                            _ptr(dpoints), _ptr(dvertices), _stream(dev))
    _check(rc, "mr_nearest_triangle_backward")
    return dpoints, dvertices


def winding_number_plan(B, N, T):
    """The launch shape mr_winding_number_forward takes for B images of N queries against T triangles, a pure host
    function: {"splits", "queries_per_lane", "triangle_tile", "workgroup_size"} (include/mesh_raster.h).  T above
    2^24 is refused: the fixed-point sum could leave the 64-bit range."""
    return _plan("winding_number_plan", (B, N, T),
                 ("splits", "queries_per_lane", "triangle_tile", "workgroup_size"),
                 "1..65535 images of 1..2^28 points and 1..2^24 triangles")


def winding_number_forward(points, vertices, triangles, lengths=None):
    """points [B,N,3], vertices [B,V,3] f32, triangles [T,3] i32, lengths [B] i32 or None (device) -> w [B,N] f32, the
    generalized winding number of the mesh around every valid query (0 in padded rows): mr_winding_number_forward."""
    B, N, V, T = _chk_point_mesh(points, vertices, triangles, lengths)
    if T > 1 << 24:
        raise ValueError("the winding number takes at most 2^24 triangles, got %d" % T)
    dev = _require_device(points, vertices, triangles, *([lengths] if lengths is not None else []))
    L = lib()
    points, vertices, triangles = points.contiguous(), vertices.contiguous(), triangles.contiguous()
    lengths = lengths.contiguous() if lengths is not None else None
    w = torch.empty(B, N, dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        ws, have = _workspace(dev, L.mr_winding_number_workspace_bytes(B, N, T))
        rc = L.mr_winding_number_forward(_ptr(points), _ptr(vertices), _ptr(triangles), _ptr(lengths), B, N, V, T,
                                         _ptr(w), _ptr(ws), have, _stream(dev))
    _check(rc, "mr_winding_number_forward")
    return w


def cast_rays_plan(B, N, T):
    """The launch shape mr_cast_rays_forward takes for B images of N rays against T triangles, a pure host function:
    {"splits", "queries_per_lane", "triangle_tile", "workgroup_size"} (include/mesh_raster.h).  The size limits are
    the winding number's."""
    return _plan("cast_rays_plan", (B, N, T), ("splits", "queries_per_lane", "triangle_tile", "workgroup_size"),
                 "1..65535 images of 1..2^28 rays and 1..2^24 triangles")


def _chk_rays(origins, directions, vertices, triangles, lengths):
    B, N, V, T = _chk_point_mesh(origins, vertices, triangles, lengths)
    _chk("directions", directions, _F32, B, N, 3)
    if T > 1 << 24:
        raise ValueError("ray casting takes at most 2^24 triangles, got %d" % T)
    return B, N, V, T


def cast_rays_forward(origins, directions, vertices, triangles, lengths=None, t_min=0.0, t_max=float("inf")):
    """origins, directions [B,N,3], vertices [B,V,3] f32, triangles [T,3] i32, lengths [B] i32 or None (device) ->
    (t [B,N] f32, face [B,N] i32, bary [B,N,3] f32), +inf / -1 / 0 for a ray without a hit: mr_cast_rays_forward."""
    B, N, V, T = _chk_rays(origins, directions, vertices, triangles, lengths)
    if not 0.0 <= t_min <= t_max:
        raise ValueError("0 <= t_min <= t_max is required, got %r and %r" % (t_min, t_max))
    dev = _require_device(origins, directions, vertices, triangles, *([lengths] if lengths is not None else []))
    L = lib()
    origins, directions = origins.contiguous(), directions.contiguous()
    vertices, triangles = vertices.contiguous(), triangles.contiguous()
    lengths = lengths.contiguous() if lengths is not None else None
    t = torch.empty(B, N, dtype=_F32, device=dev)
    face = torch.empty(B, N, dtype=_I32, device=dev)
    bary = torch.empty(B, N, 3, dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        ws, have = _workspace(dev, L.mr_cast_rays_workspace_bytes(B, N, T))
        rc = L.mr_cast_rays_forward(_ptr(origins), _ptr(directions), _ptr(vertices), _ptr(triangles), _ptr(lengths), B,
                                    N, V, T, float(t_min), float(t_max), _ptr(t), _ptr(face), _ptr(bary), _ptr(ws),
                                    have, _stream(dev))
    _check(rc, "mr_cast_rays_forward")
    return t, face, bary


def cast_rays_backward(directions, vertices, triangles, lengths, t, face, bary, grad_t, index=None, want_dorigins=True,
                       want_ddirections=True, want_dvertices=True):
    """mr_cast_rays_backward -> (dorigins [B,N,3], ddirections [B,N,3], dvertices [B,V,3]), None for what is not
    wanted.  index: (order [B,3N], offsets [B,V+1]), nearest_inverted_index() of the (ray, corner) entries' vertices,
    needed for dvertices."""
    B, N, V, T = _chk_rays(directions, directions, vertices, triangles, lengths)   # the backward takes no origins
    _chk("t", t, _F32, B, N)
    _chk("face", face, _I32, B, N)
    _chk("bary", bary, _F32, B, N, 3)
    _chk("upstream gradient", grad_t, _F32, B, N)
    tensors = [directions, vertices, triangles, t, face, bary, grad_t] + ([lengths] if lengths is not None else [])
    if index is not None:
        _chk("order", index[0], _I32, B, 3 * N)
        _chk("offsets", index[1], _I32, B, V + 1)
        tensors += list(index)
    elif want_dvertices:
        raise ValueError("dvertices needs the inverted index of the named corners")
    dev = _require_device(*tensors)
    L = lib()
    c = lambda x: x.contiguous() if x is not None else None
    order, offsets = index if index is not None else (None, None)
    dorigins = torch.empty(B, N, 3, dtype=_F32, device=dev) if want_dorigins else None
    ddirections = torch.empty(B, N, 3, dtype=_F32, device=dev) if want_ddirections else None
    dvertices = torch.empty(B, V, 3, dtype=_F32, device=dev) if want_dvertices else None
    held = [c(x) for x in (directions, vertices, triangles, lengths, t, face, bary, order, offsets, grad_t)]
    with torch.cuda.device(dev):
        rc = L.mr_cast_rays_backward(*[_ptr(x) for x in held[:4]], B, N, V, T, *[_ptr(x) for x in held[4:]],
                                     _ptr(dorigins), _ptr(ddirections), _ptr(dvertices), _stream(dev))
    _check(rc, "mr_cast_rays_backward")
    return dorigins, ddirections, dvertices


def nearest_point_of_triangle_plan(B, N, T):
    """The launch shape mr_nearest_point_of_triangle_forward takes for B images of T triangles against N points, a
    pure host function: {"splits", "points_per_step", "point_tile", "workgroup_size"} (include/mesh_raster.h)."""
    return _plan("nearest_point_of_triangle_plan", (B, N, T),
                 ("splits", "points_per_step", "point_tile", "workgroup_size"),
                 "1..65535 images of 1..2^28 points and triangles")


def nearest_point_of_triangle_forward(points, vertices, triangles, lengths=None, want_sqdist=True, want_total=False):
    """points [B,N,3], vertices [B,V,3] f32, triangles [T,3] i32, lengths [B] i32 or None (device) -> (sqdist [B,T]
    f32 or None, index [B,T] i32, bary [B,T,3] f32, total [B] f32 or None: the mean of sqdist over the usable
    triangles, usable [B] i32 or None: their count, formed on the device): mr_nearest_point_of_triangle_forward."""
    B, N, V, T = _chk_point_mesh(points, vertices, triangles, lengths)
    dev = _require_device(points, vertices, triangles, *([lengths] if lengths is not None else []))
    L = lib()
    points, vertices, triangles = points.contiguous(), vertices.contiguous(), triangles.contiguous()
    lengths = lengths.contiguous() if lengths is not None else None
    sqdist = torch.empty(B, T, dtype=_F32, device=dev) if want_sqdist else None
    index = torch.empty(B, T, dtype=_I32, device=dev)
    bary = torch.empty(B, T, 3, dtype=_F32, device=dev)
    total = torch.empty(B, dtype=_F32, device=dev) if want_total else None
    usable = torch.empty(B, dtype=_I32, device=dev) if want_total else None
    with torch.cuda.device(dev):
        ws, have = _workspace(dev, L.mr_nearest_point_of_triangle_workspace_bytes(B, N, T))
        rc = L.mr_nearest_point_of_triangle_forward(_ptr(points), _ptr(vertices), _ptr(triangles), _ptr(lengths), B, N,
                                                    V, T, _ptr(sqdist), _ptr(index), _ptr(bary), _ptr(total),
                                                    _ptr(usable), _ptr(ws), have, _stream(dev))
    _check(rc, "mr_nearest_point_of_triangle_forward")
    return sqdist, index, bary, total, usable


def nearest_point_of_triangle_backward(points, vertices, triangles, lengths, index, bary, corner_index=None,
                                       point_index=None, grad_triangles=None, grad_images=None, usable=None,
                                       want_dpoints=True, want_dvertices=True):
    """mr_nearest_point_of_triangle_backward -> (dpoints [B,N,3] or None, dvertices [B,V,3] or None).  corner_index:
    (order [B,3T], offsets [B,V+1]), nearest_inverted_index() of the (triangle, corner) entries' vertices, needed for
    dvertices; point_index: (order [B,T], offsets [B,N+1]), that of index, needed for dpoints; usable [B] i32: the
    forward's count, needed with grad_images."""
    B, N, V, T = _chk_point_mesh(points, vertices, triangles, lengths)
    _chk("index", index, _I32, B, T)
    _chk("bary", bary, _F32, B, T, 3)
    tensors = [points, vertices, triangles, index, bary] + ([lengths] if lengths is not None else [])
    if corner_index is not None:
        _chk("corner order", corner_index[0], _I32, B, 3 * T)
        _chk("corner offsets", corner_index[1], _I32, B, V + 1)
        tensors += list(corner_index)
    if point_index is not None:
        _chk("point order", point_index[0], _I32, B, T)
        _chk("point offsets", point_index[1], _I32, B, N + 1)
        tensors += list(point_index)
    if grad_triangles is not None:
        _chk("upstream gradient", grad_triangles, _F32, B, T)
        tensors.append(grad_triangles)
    if grad_images is not None:
        _chk("upstream gradient", grad_images, _F32, B)
        tensors.append(grad_images)
    if usable is not None:
        _chk("usable", usable, _I32, B)
        tensors.append(usable)
    dev = _require_device(*tensors)
    L = lib()
    c = lambda t: t.contiguous() if t is not None else None
    corner_order, corner_offsets = corner_index if corner_index is not None else (None, None)
    point_order, point_offsets = point_index if point_index is not None else (None, None)
    dpoints = torch.empty(B, N, 3, dtype=_F32, device=dev) if want_dpoints else None
    dvertices = torch.empty(B, V, 3, dtype=_F32, device=dev) if want_dvertices else None
    held = [c(t) for t in (points, vertices, triangles, lengths, index, bary, corner_order, corner_offsets, point_order,
                           point_offsets, grad_triangles, grad_images, usable)]
    with torch.cuda.device(dev):
        rc = L.mr_nearest_point_of_triangle_backward(*[_ptr(t) for t in held[:4]], B, N, V, T,
                                                     *[_ptr(t) for t in held[4:]], _ptr(dpoints), _ptr(dvertices),
                                                     _stream(dev))
    _check(rc, "mr_nearest_point_of_triangle_backward")
    return dpoints, dvertices


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _chk_antialias(image, ids, bary, z, clip, triangles, opposite):
    _chk("image", image, _F32, None, None, None, None)
    B, H, W, C = image.shape
    if C < 1:
        raise ValueError("image must have at least one channel, got shape %s" % list(image.shape))
    _chk("triangle ids", ids, _I32, B, H, W)
    _chk("barycentrics", bary, _F32, B, H, W, 3)
    _chk("z", z, _F32, B, H, W)
    _chk("clip-space vertices", clip, _F32, B, None, 4)
    _chk("triangles", triangles, _I32, None, 3)
    _chk("opposite", opposite, _I32, triangles.shape[0], 3)
    return B, H, W, C


def antialias_forward(image, ids, bary, z, clip, triangles, opposite, want_pair_mask=False):
    """image [B,H,W,C] -> antialiased image [B,H,W,C] (and the pair mask [B,H,W] u8 when asked for:
    bit k = left, right, down, up pair blended into this pixel)."""
    B, H, W, C = _chk_antialias(image, ids, bary, z, clip, triangles, opposite)
    dev = _require_device(image, ids, bary, z, clip, triangles, opposite)
    L = lib()
    image, ids, bary, z = _aligned16(image.contiguous()), ids.contiguous(), bary.contiguous(), z.contiguous()
    clip, triangles, opposite = _aligned16(clip.contiguous()), triangles.contiguous(), opposite.contiguous()
    V, T = clip.shape[1], triangles.shape[0]
    out = torch.empty_like(image)
    mask = torch.empty(B, H, W, dtype=_U8, device=dev) if want_pair_mask else None
    with torch.cuda.device(dev):
        rc = L.mr_antialias_forward(_ptr(image), _ptr(ids), _ptr(bary), _ptr(z), _ptr(clip), _ptr(triangles),
                                    _ptr(opposite), B, V, T, W, H, C, _ptr(out), _ptr(mask), _stream(dev))
    _check(rc, "mr_antialias_forward")
    return (out, mask) if want_pair_mask else out


def antialias_backward(dout, image, ids, bary, z, clip, triangles, opposite):
    """-> (dimage [B,H,W,C], dclip [B,V,4])."""
    B, H, W, C = _chk_antialias(image, ids, bary, z, clip, triangles, opposite)
    _chk("upstream gradient", dout, _F32, B, H, W, C)
    dev = _require_device(dout, image, ids, bary, z, clip, triangles, opposite)
    L = lib()
    dout, image = _aligned16(dout.contiguous()), image.contiguous()
    ids, bary, z = ids.contiguous(), bary.contiguous(), z.contiguous()
    clip, triangles, opposite = _aligned16(clip.contiguous()), triangles.contiguous(), opposite.contiguous()
    V, T = clip.shape[1], triangles.shape[0]
    dimage = torch.empty_like(dout)
    dclip = torch.empty(B, V, 4, dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        need = L.mr_antialias_backward_workspace_bytes(B, V, T, W, H, C)
        ws, have = _workspace(dev, need)
        _sync_deterministic()
        rc = L.mr_antialias_backward(_ptr(dout), _ptr(image), _ptr(ids), _ptr(bary), _ptr(z), _ptr(clip),
                                     _ptr(triangles), _ptr(opposite), B, V, T, W, H, C, _ptr(dimage),
                                     _ptr(dclip), _ptr(ws), have, _stream(dev))
    _check(rc, "mr_antialias_backward")
    return dimage, dclip


def _pixel_stride(normals, diffuse):
    """The pixel stride C when normals and diffuse are two disjoint three-channel slices of one contiguous
    [B,H,W,C] buffer (rasterize()'s packed attributes), else None.  Returns (C, normals' channel, diffuse's
    channel)."""
    B, H, W, _ = normals.shape
    if normals.untyped_storage().data_ptr() != diffuse.untyped_storage().data_ptr():
        return None
    C = normals.stride(2)
    for t in (normals, diffuse):
        want = (H * W * C, W * C, C, 1)
        if any(n > 1 and st != w for n, st, w in zip(t.shape, t.stride(), want)):
            return None
    on, od = normals.storage_offset(), diffuse.storage_offset()
    cn, cd = on % C, od % C
    if C < 6 or on - cn != od - cd or cn + 3 > C or cd + 3 > C or abs(cn - cd) < 3:
        return None
    return C, cn, cd


def _chk_sh(normals, diffuse, alphas, sh):
    _chk("normals", normals, _F32, None, None, None, 3)
    B, H, W, _ = normals.shape
    _chk("diffuse colors", diffuse, _F32, B, H, W, 3)
    if alphas is not None:
        _chk("alphas", alphas, _F32, B, H, W)
    _chk("sh coefficients", sh, _F32, B, 9, 3)
    if B > 65535 or H * W > 1 << 30:
        raise ValueError("spherical-harmonics shading takes at most 65535 images of at most 2^30 pixels, got %s"
                         % list(normals.shape))
    return B, H, W


def _sh_inputs(normals, diffuse, alphas, sh):
    """-> (normals, diffuse, pixel stride, packed channels or None, alphas, sh) as the kernels read them: a packed
    pair goes through as it is, anything else is made contiguous."""
    packed = _pixel_stride(normals, diffuse)
    if packed is None:
        normals, diffuse, stride = normals.contiguous(), diffuse.contiguous(), 3
    else:
        stride = packed[0]
    alphas = alphas.contiguous() if alphas is not None else None
    return normals, diffuse, stride, packed, alphas, sh.contiguous()


def sh_shade_forward(normals, diffuse, alphas, sh, flip=True):
    """normals, diffuse [B,H,W,3] f32 (two channel slices of one contiguous [B,H,W,C] buffer are read in place),
    alphas [B,H,W] f32 or None (alpha = any(diffuse >= 0)), sh [B,9,3] f32 -> RGBA [B,H,W,4], rows flipped when
    `flip` ("Spherical-harmonics lighting")."""
    B, H, W = _chk_sh(normals, diffuse, alphas, sh)
    dev = _require_device(*[t for t in (normals, diffuse, alphas, sh) if t is not None])
    L = lib()
    normals, diffuse, stride, _, alphas, sh = _sh_inputs(normals, diffuse, alphas, sh)
    rgba = torch.empty(B, H, W, 4, dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        rc = L.mr_sh_shade_forward(_ptr(normals), _ptr(diffuse), stride, _ptr(alphas), _ptr(sh), B, W, H,
                                   1 if flip else 0, _ptr(rgba), _stream(dev))
    _check(rc, "mr_sh_shade_forward")
    return rgba


def sh_shade_backward(drgba, normals, diffuse, alphas, sh, flip=True, want_normals=True, want_diffuse=True,
                      want_alphas=True, want_sh=True, packed_grad=False):
    """-> (dnormals, ddiffuse, dalphas, dsh); an unwanted gradient is None, and so is dalphas when alphas is None.
    When normals and diffuse are read in place from one [B,H,W,C] buffer, dnormals and ddiffuse are the same
    channel slices of one [B,H,W,C] gradient (its other channels zero); with packed_grad=True that buffer is
    returned in their place: (dpacked, dalphas, dsh)."""
    B, H, W = _chk_sh(normals, diffuse, alphas, sh)
    _chk("upstream gradient", drgba, _F32, B, H, W, 4)
    dev = _require_device(*[t for t in (drgba, normals, diffuse, alphas, sh) if t is not None])
    L = lib()
    normals, diffuse, stride, packed, alphas, sh = _sh_inputs(normals, diffuse, alphas, sh)
    drgba = _aligned16(drgba.contiguous())
    want_alphas = want_alphas and alphas is not None
    dpacked = None
    if packed is not None and (want_normals or want_diffuse or packed_grad):
        C, cn, cd = packed
        covered = C == 6 and want_normals and want_diffuse
        dpacked = (torch.empty if covered else torch.zeros)(B, H, W, C, dtype=_F32, device=dev)
        dnormals = dpacked[..., cn:cn + 3] if want_normals else None
        ddiffuse = dpacked[..., cd:cd + 3] if want_diffuse else None
    else:
        dnormals = torch.empty(B, H, W, 3, dtype=_F32, device=dev) if want_normals else None
        ddiffuse = torch.empty(B, H, W, 3, dtype=_F32, device=dev) if want_diffuse else None
    dalphas = torch.empty(B, H, W, dtype=_F32, device=dev) if want_alphas else None
    dsh = torch.empty(B, 9, 3, dtype=_F32, device=dev) if want_sh else None
    with torch.cuda.device(dev):
        ws, have = None, 0
        if want_sh:
            ws, have = _workspace(dev, L.mr_sh_shade_backward_workspace_bytes(B, W, H))
        rc = L.mr_sh_shade_backward(_ptr(drgba), _ptr(normals), _ptr(diffuse), stride, _ptr(alphas), _ptr(sh), B, W,
                                    H, 1 if flip else 0, _ptr(dnormals), _ptr(ddiffuse), _ptr(dalphas), _ptr(dsh),
                                    _ptr(ws), have, _stream(dev))
    _check(rc, "mr_sh_shade_backward")
    if packed_grad and dpacked is not None:
        return dpacked, dalphas, dsh
    return dnormals, ddiffuse, dalphas, dsh


TEXTURE_BOUNDARY = {"wrap": 0, "clamp": 1}   # mesh_raster.h, MR_TEXTURE_WRAP / MR_TEXTURE_CLAMP


def _chk_texture(tex, uv, mask, boundary_mode):
    """-> (B, H, W, Ht, Wt, C, tex_batched, boundary code)."""
    _chk("uv", uv, _F32, None, None, None, 2)
    B, H, W, _ = uv.shape
    if torch.is_tensor(tex) and tex.dim() == 4:
        _chk("texture", tex, _F32, B, None, None, None)
    else:
        _chk("texture", tex, _F32, None, None, None)
    Ht, Wt, C = tex.shape[-3:]
    if not 1 <= C <= 4 or Ht < 1 or Wt < 1:
        raise ValueError("texture must have 1 to 4 channels and at least one texel, got shape %s" % list(tex.shape))
    if mask is not None:
        _chk("mask", mask, _F32, B, H, W)
    if boundary_mode not in TEXTURE_BOUNDARY:
        raise ValueError("boundary_mode must be 'wrap' or 'clamp', got %r" % (boundary_mode,))
    tiles = ((W + 63) // 64) * ((H + 15) // 16)   # the backward's 64 x 16 pixel tiles
    if B > 65535 or H * W > 1 << 30 or tiles > 1 << 22 or Ht > 65536 or Wt > 65536 or Ht * Wt > 1 << 28:
        raise ValueError("texture sampling takes at most 65535 images of at most 2^30 pixels (and at most 2^22 tiles "
                         "of 64 x 16 pixels) and textures of at most 65536 x 65536, 2^28 texels; got uv %s, texture %s"
                         % (list(uv.shape), list(tex.shape)))
    return B, H, W, Ht, Wt, C, int(tex.dim() == 4), TEXTURE_BOUNDARY[boundary_mode]


def texture_forward(tex, uv, mask=None, boundary_mode="wrap"):
    """tex [Ht,Wt,C] or [B,Ht,Wt,C] f32 (1 <= C <= 4), uv [B,H,W,2] f32, mask [B,H,W] f32 or None -> [B,H,W,C]
    bilinear samples ("Texture mapping")."""
    B, H, W, Ht, Wt, C, batched, boundary = _chk_texture(tex, uv, mask, boundary_mode)
    dev = _require_device(*[t for t in (tex, uv, mask) if t is not None])
    L = lib()
    tex, uv = _aligned16(tex.contiguous()), _aligned16(uv.contiguous())
    mask = mask.contiguous() if mask is not None else None
    out = torch.empty(B, H, W, C, dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        rc = L.mr_texture_forward(_ptr(tex), _ptr(uv), _ptr(mask), batched, Ht, Wt, C, B, W, H, boundary, _ptr(out),
                                  _stream(dev))
    _check(rc, "mr_texture_forward")
    return out


def texture_backward(dout, tex, uv, mask=None, boundary_mode="wrap", want_tex=True, want_uv=True):
    """-> (dtex with tex's shape, duv [B,H,W,2]); an unwanted gradient is None.  A shared texture's gradient is
    summed over the batch."""
    B, H, W, Ht, Wt, C, batched, boundary = _chk_texture(tex, uv, mask, boundary_mode)
    _chk("upstream gradient", dout, _F32, B, H, W, C)
    dev = _require_device(*[t for t in (dout, tex, uv, mask) if t is not None])
    L = lib()
    dout = _aligned16(dout.contiguous())
    tex, uv = _aligned16(tex.contiguous()), _aligned16(uv.contiguous())
    mask = mask.contiguous() if mask is not None else None
    dtex = torch.empty(tex.shape, dtype=_F32, device=dev) if want_tex else None
    duv = torch.empty(B, H, W, 2, dtype=_F32, device=dev) if want_uv else None
    if B == 0 or not (want_tex or want_uv):
        return (dtex.zero_() if dtex is not None else None), duv
    with torch.cuda.device(dev):
        _sync_deterministic()
        ws, have = None, 0
        if want_tex:
            ws, have = _workspace(dev, L.mr_texture_backward_workspace_bytes(batched, Ht, Wt, C, B, W, H))
        rc = L.mr_texture_backward(_ptr(dout), _ptr(tex), _ptr(uv), _ptr(mask), batched, Ht, Wt, C, B, W, H,
                                   boundary, _ptr(dtex), _ptr(duv), _ptr(ws), have, _stream(dev))
    _check(rc, "mr_texture_backward")
    return dtex, duv


def _max_level_code(max_mip_level):
    """None -> -1 (no cap); otherwise a non-negative integer."""
    if max_mip_level is None:
        return -1
    if isinstance(max_mip_level, bool) or not isinstance(max_mip_level, int) or max_mip_level < 0:
        raise ValueError("max_mip_level must be None or a non-negative integer, got %r" % (max_mip_level,))
    return min(max_mip_level, 64)


def texture_mip_levels(Ht, Wt, max_mip_level=None):
    """The number of pyramid levels of an Ht x Wt texture: 1 + min(tz(Ht), tz(Wt), max_mip_level).  Needs no GPU."""
    if not (1 <= Ht <= 65536 and 1 <= Wt <= 65536):
        raise ValueError("texture extents must be in 1 .. 65536, got %r x %r" % (Ht, Wt))
    return lib().mr_texture_mip_levels(int(Ht), int(Wt), _max_level_code(max_mip_level))


def _chk_texture_mip(tex, uv, uv_da, mask, boundary_mode, max_mip_level):
    out = _chk_texture(tex, uv, mask, boundary_mode)
    B, H, W = out[:3]
    _chk("uv_da", uv_da, _F32, B, H, W, 4)
    return out + (_max_level_code(max_mip_level),)


def _mip_pyramid_views(pyramid, tex, levels):
    """The packed pyramid buffer as a list of [Bt,Hl,Wl,C] views, levels 1 .. L-1."""
    Ht, Wt, C = tex.shape[-3:]
    count = tex.shape[0] if tex.dim() == 4 else 1
    per = pyramid.view(count, -1) if pyramid.numel() else pyramid
    out, off = [], 0
    for l in range(1, levels):
        h, w = Ht >> l, Wt >> l
        out.append(per[:, off * C:(off + h * w) * C].reshape(count, h, w, C))
        off += h * w
    return out


def texture_mip_forward(tex, uv, uv_da, mask=None, boundary_mode="wrap", max_mip_level=None):
    """tex [Ht,Wt,C] or [B,Ht,Wt,C] f32, uv [B,H,W,2], uv_da [B,H,W,4] f32, mask [B,H,W] f32 or None ->
    (out [B,H,W,C], pyramid): mipmapped trilinear samples ("Texture mapping") and the packed
    pyramid levels >= 1 (a flat float32 tensor, empty when there is one level) that texture_mip_backward reads."""
    B, H, W, Ht, Wt, C, batched, boundary, cap = _chk_texture_mip(tex, uv, uv_da, mask, boundary_mode, max_mip_level)
    dev = _require_device(*[t for t in (tex, uv, uv_da, mask) if t is not None])
    L = lib()
    tex, uv, uv_da = _aligned16(tex.contiguous()), _aligned16(uv.contiguous()), _aligned16(uv_da.contiguous())
    mask = mask.contiguous() if mask is not None else None
    out = torch.empty(B, H, W, C, dtype=_F32, device=dev)
    pyramid = torch.empty(L.mr_texture_mip_pyramid_bytes(batched, Ht, Wt, C, B, cap) // 4, dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        rc = L.mr_texture_mip_forward(_ptr(tex), _ptr(uv), _ptr(uv_da), _ptr(mask), batched, Ht, Wt, C, B, W, H,
                                      boundary, cap, _ptr(pyramid) if pyramid.numel() else ctypes.c_void_p(0),
                                      _ptr(out), _stream(dev))
    _check(rc, "mr_texture_mip_forward")
    return out, pyramid


def texture_mip_pyramid(tex, max_mip_level=None):
    """tex [Ht,Wt,C] or [Bt,Ht,Wt,C] f32 -> the pyramid levels 1 .. L-1 as a list of [Bt,Hl,Wl,C] tensors (Bt = 1
    for a shared texture), built by the kernel texture_mip_forward uses."""
    batched = torch.is_tensor(tex) and tex.dim() == 4
    B = tex.shape[0] if batched else 1
    uv = torch.zeros(B, 1, 1, 2, dtype=_F32, device=tex.device)
    uv_da = torch.zeros(B, 1, 1, 4, dtype=_F32, device=tex.device)
    _, pyramid = texture_mip_forward(tex, uv, uv_da, None, "wrap", max_mip_level)
    return _mip_pyramid_views(pyramid, tex, texture_mip_levels(tex.shape[-3], tex.shape[-2], max_mip_level))


def texture_mip_backward(dout, tex, pyramid, uv, uv_da, mask=None, boundary_mode="wrap", max_mip_level=None,
                         want_tex=True, want_uv=True):
    """-> (dtex with tex's shape, duv [B,H,W,2]); an unwanted gradient is None.  pyramid: texture_mip_forward's."""
    B, H, W, Ht, Wt, C, batched, boundary, cap = _chk_texture_mip(tex, uv, uv_da, mask, boundary_mode, max_mip_level)
    _chk("upstream gradient", dout, _F32, B, H, W, C)
    L = lib()
    _chk("pyramid", pyramid, _F32, L.mr_texture_mip_pyramid_bytes(batched, Ht, Wt, C, B, cap) // 4)
    dev = _require_device(*[t for t in (dout, tex, pyramid, uv, uv_da, mask) if t is not None])
    dout = _aligned16(dout.contiguous())
    tex, uv, uv_da = _aligned16(tex.contiguous()), _aligned16(uv.contiguous()), _aligned16(uv_da.contiguous())
    pyramid = _aligned16(pyramid.contiguous())
    mask = mask.contiguous() if mask is not None else None
    dtex = torch.empty(tex.shape, dtype=_F32, device=dev) if want_tex else None
    duv = torch.empty(B, H, W, 2, dtype=_F32, device=dev) if want_uv else None
    if B == 0 or not (want_tex or want_uv):
        return (dtex.zero_() if dtex is not None else None), duv
    with torch.cuda.device(dev):
        _sync_deterministic()
        ws, have = None, 0
        if want_tex:
            ws, have = _workspace(dev, L.mr_texture_mip_backward_workspace_bytes(batched, Ht, Wt, C, B, W, H, cap))
        rc = L.mr_texture_mip_backward(_ptr(dout), _ptr(tex), _ptr(pyramid) if pyramid.numel() else ctypes.c_void_p(0),
                                       _ptr(uv), _ptr(uv_da), _ptr(mask), batched, Ht, Wt, C, B, W, H, boundary, cap,
                                       _ptr(dtex), _ptr(duv), _ptr(ws), have, _stream(dev))
    _check(rc, "mr_texture_mip_backward")
    return dtex, duv


def attribute_derivatives(ids, bary, clip, triangles, attributes, attribute_triangles=None):
    """ids [B,H,W] i32, bary [B,H,W,3], clip [B,V,4], triangles [T,3] i32, attributes [B,Va,A] f32 (1 <= A <= 4),
    attribute_triangles [T,3] i32 or None (then Va = V) -> [B,H,W,A,2] f32: the screen-space derivatives
    (d a / d X, d a / d Y) of the perspective-correct interpolation per pixel step, 0 on the background."""
    B, V, T = _chk_mesh(clip, triangles)
    H, W = _chk_gbuffer(ids, bary, B)
    _chk("attributes", attributes, _F32, B, None, None)
    Va, A = attributes.shape[1], attributes.shape[2]
    if not 1 <= A <= 4:
        raise ValueError("attribute_derivatives takes 1 to 4 attributes, got %d" % A)
    if attribute_triangles is not None:
        _chk("attribute_triangles", attribute_triangles, _I32, T, 3)
    elif Va != V:
        raise ValueError("attributes must have one row per vertex when attribute_triangles is None")
    if T < 1 or V < 1 or Va < 1 or B > 65535 or H * W > 1 << 30:
        raise ValueError("attribute_derivatives needs at least one triangle and vertex, at most 65535 images of at "
                         "most 2^30 pixels")
    dev = _require_device(*[t for t in (ids, bary, clip, triangles, attributes, attribute_triangles) if t is not None])
    L = lib()
    ids, bary, clip = ids.contiguous(), bary.contiguous(), _aligned16(clip.contiguous())
    triangles, attributes = triangles.contiguous(), attributes.contiguous()
    attribute_triangles = attribute_triangles.contiguous() if attribute_triangles is not None else None
    out = torch.empty(B, H, W, A, 2, dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        rc = L.mr_attribute_derivatives(_ptr(ids), _ptr(bary), _ptr(clip), _ptr(triangles), _ptr(attributes),
                                        _ptr(attribute_triangles), B, V, T, Va, W, H, A, _ptr(out), _stream(dev))
    _check(rc, "mr_attribute_derivatives")
    return out


def shade_backward(drgba, ids, bary, clip, normals, positions, diffuse, triangles, light_positions,
                   light_intensities, ambient, corner_records=None, adjacency=None, l1_signs=None,
                   transforms=None, want_light_grads=True, want_normal_grads=True, want_diffuse_grads=True,
                   normalised_gbuffer=False, want_clip_grads=True, prepared=None, empty_regions=None,
                   private_gbuffer=False):
    """_shade_backward_call for any light count up to shade_max_lights().  The kernels keep the light
    gradients' 6 L sums in registers, four lights per call; with more lights the vertex-side gradients
    come from one call over all lights (a run-time loop, no light gradients) and each group of four
    lights gets a call of its own for d light_positions / d light_intensities -- a light's gradient
    depends on that light, the upstream gradient and the pixel's attributes, not on the other lights.
    (1 + ceil(L / 4) passes over the G-buffer: more than four lights WITH light gradients is the rare
    case -- the reference's tests and examples use one to three.)"""
    nl = light_positions.shape[1]
    kw = dict(corner_records=corner_records, adjacency=adjacency, l1_signs=l1_signs, transforms=transforms,
              want_normal_grads=want_normal_grads, want_diffuse_grads=want_diffuse_grads,
              normalised_gbuffer=normalised_gbuffer, want_clip_grads=want_clip_grads, prepared=prepared,
              empty_regions=empty_regions, private_gbuffer=private_gbuffer)
    fast = shade_fast_lights() if nl > 4 else nl
    if nl <= fast or not want_light_grads:
        return _shade_backward_call(drgba, ids, bary, clip, normals, positions, diffuse, triangles,
                                    light_positions, light_intensities, ambient, want_light_grads=want_light_grads,
                                    **kw)
    out = _shade_backward_call(drgba, ids, bary, clip, normals, positions, diffuse, triangles, light_positions,
                               light_intensities, ambient, want_light_grads=False, **kw)
    chunk_kw = dict(kw, want_normal_grads=False, want_diffuse_grads=False) if adjacency is not None else kw
    dlpos, dlint, damb = [], [], None
    for first in range(0, nl, fast):
        part = _shade_backward_call(drgba, ids, bary, clip, normals, positions, diffuse, triangles,
                                    light_positions[:, first:first + fast].contiguous(),
                                    light_intensities[:, first:first + fast].contiguous(),
                                    ambient if first == 0 else None, want_light_grads=True, **chunk_kw)
        dlpos.append(part[4])
        dlint.append(part[5])
        if first == 0:
            damb = part[6]
    return out[:4] + (torch.cat(dlpos, 1), torch.cat(dlint, 1), damb)


def _shade_backward_call(drgba, ids, bary, clip, normals, positions, diffuse, triangles, light_positions,
                         light_intensities, ambient, corner_records=None, adjacency=None, l1_signs=None,
                         transforms=None, want_light_grads=True, want_normal_grads=True, want_diffuse_grads=True,
                         normalised_gbuffer=False, want_clip_grads=True, prepared=None, empty_regions=None,
                         private_gbuffer=False):
    """-> (dclip [B,V,4], dnormals, dpositions, ddiffuse [B,V,3], dlight_positions,
    dlight_intensities [B,L,3], dambient [B,3] or None); with want_light_grads=False the last three
    are None and the kernel leaves their accumulation out; want_normal_grads / want_diffuse_grads=False
    (needs `adjacency`) return None for that gradient and its sums are not formed either -- the
    backward then runs the lane-accumulating kernel (18 or 27 sums per triangle instead of 36).

    transforms ([B,4,4], needs `adjacency`): clip = transforms . (positions, 1); dpositions then also
    holds the clip-space gradient pulled back through that product (the whole d / d world vertices).

    l1_signs: the packed sign codes of l1_loss_forward(rgba, target); `drgba` is then the 1-element
    upstream gradient of that loss and the [B,H,W,4] gradient image is never materialised.

    normalised_gbuffer: ids / bary are what rasterize_forward / render_forward wrote for these vertices
    (MR_GBUFFER_NORMALISED): the pixel pass leaves the alpha terms out, same bits.

    want_clip_grads=False (needs `transforms`): dclip is returned as None -- the caller differentiates to
    the world-space vertices only; the pull-back through the transforms is then folded into the pixel
    pass where the library has that variant (9 sums per triangle instead of 18).

    prepared: the block render_forward(..., prepare_backward=True) returned for these inputs (or None).
    empty_regions: render_forward(..., want_empty_regions=True)'s map for this G-buffer (or None).

    private_gbuffer: ids and prepared are what render_forward(..., private_gbuffer=True) returned (MR_GBUFFER_PRIVATE);
    bary is None.  Sign-coded upstream, vertex gradients only, one to four lights: anything else is refused."""
    if private_gbuffer:
        if bary is not None or prepared is None or l1_signs is None or not normalised_gbuffer:
            raise ValueError("a private G-buffer has no barycentrics and comes with its prepared block and sign codes")
        _chk("triangle ids", ids, _I32, clip.shape[0], None, None)
        if prepared.numel() < lib().mr_render_forward_l1_private_bytes(clip.shape[0], triangles.shape[0], ids.shape[2], ids.shape[1]):
            raise ValueError("prepared must be the block render_forward(private_gbuffer=True) returned for these inputs")
        bary = ids   # (stands in below where every tensor is checked; not passed on)
    if empty_regions is not None:
        _chk("empty_regions", empty_regions, _U8, clip.shape[0], (ids.shape[1] + 63) // 64, (ids.shape[2] + 63) // 64)
        empty_regions = empty_regions.contiguous()
    if prepared is not None and (prepared.dtype != torch.uint8 or
                                 prepared.numel() < lib().mr_shade_backward_prepared_bytes(clip.shape[0], triangles.shape[0])):
        raise ValueError("prepared must be the block render_forward(prepare_backward=True) returned for these inputs")
    if not want_clip_grads and transforms is None:
        raise ValueError("without transforms the clip-space gradient is the vertex gradient: it cannot be left out")
    tensors = [drgba, ids, bary, clip, normals, positions, diffuse, triangles, light_positions,
               light_intensities]
    B, V, _ = _chk_mesh(clip, triangles)
    for name, t in (("normals", normals), ("positions", positions), ("diffuse colors", diffuse)):
        _chk(name, t, _F32, B, V, 3)
    h, w = (ids.shape[1], ids.shape[2]) if private_gbuffer else _chk_gbuffer(ids, bary, B)
    _chk_lights(light_positions, light_intensities, ambient, B, shade_max_lights())
    if l1_signs is None:
        _chk("upstream gradient", drgba, _F32, B, h, w, 4)
    else:
        _chk("upstream gradient of the loss", drgba, _F32, 1)
    if adjacency is not None:
        _chk("adjacency offsets", adjacency[0], _I32, V + 1)
        _chk("adjacency entries", adjacency[1], _I32, None)
    if transforms is not None:
        if adjacency is None:
            raise ValueError("transforms are applied by the per-vertex gather: pass the adjacency too")
        _chk("clip-space transforms", transforms, _F32, B, 4, 4)
        tensors = tensors + [transforms]
        transforms = transforms.contiguous()
    dev = _require_device(*(tensors + ([ambient] if ambient is not None else [])))
    L = lib()
    (drgba, ids, bary, clip, normals, positions, diffuse, triangles, light_positions,
     light_intensities) = [t.contiguous() for t in tensors[:10]]
    ambient = ambient.contiguous() if ambient is not None else None
    if private_gbuffer:
        bary = None
    B, H, W = ids.shape
    V, T, nl = normals.shape[1], triangles.shape[0], light_positions.shape[1]
    # one allocation, laid out back to back: the library then zeroes all outputs with one memset
    n4, n3, nlg = B * V * 4, B * V * 3, (B * (6 * nl + 3) if want_light_grads else 0)
    flat = torch.empty(n4 + 3 * n3 + nlg, dtype=torch.float32, device=dev)
    dclip = flat[:n4].view(B, V, 4)
    dn = flat[n4:n4 + n3].view(B, V, 3)
    dp = flat[n4 + n3:n4 + 2 * n3].view(B, V, 3)
    dd = flat[n4 + 2 * n3:n4 + 3 * n3].view(B, V, 3)
    lg = flat[n4 + 3 * n3:].view(B, 6 * nl + 3) if want_light_grads else None
    if adjacency is None and not (want_normal_grads and want_diffuse_grads):
        raise ValueError("leaving a gradient out needs the per-vertex gather: pass the adjacency")
    if not want_normal_grads:
        dn = None
    if not want_diffuse_grads:
        dd = None
    if not want_clip_grads:
        dclip = None
    tail = (B, V, T, W, H, nl, _ptr(dclip), _ptr(dn), _ptr(dp), _ptr(dd), _ptr(lg), _ptr(corner_records),
            _ptr(adjacency[0]) if adjacency is not None else None,
            _ptr(adjacency[1]) if adjacency is not None else None, _ptr(transforms),
            (GBUFFER_NORMALISED if normalised_gbuffer else 0) | (GBUFFER_PRIVATE if private_gbuffer else 0),
            _ptr(prepared), _ptr(empty_regions))
    with torch.cuda.device(dev):
        _arm_timer(TIMER_SHADE_BACKWARD)
        _sync_deterministic()
        L.mr_debug_set_shade_backward_kernel(_shade_backward_kernel)
        if l1_signs is not None:
            if l1_signs.dtype != torch.uint8 or l1_signs.numel() != B * H * W or drgba.numel() != 1:
                raise ValueError("l1_signs must hold one byte per pixel and drgba the scalar upstream gradient")
            need = L.mr_shade_backward_l1_workspace_bytes(B, V, T, W, H)
            ws, have = _workspace(dev, need)
            rc = L.mr_shade_backward_l1(_ptr(l1_signs.contiguous()), _ptr(drgba), _ptr(ids), _ptr(bary), _ptr(clip),
                                        _ptr(normals), _ptr(positions), _ptr(diffuse), _ptr(triangles),
                                        _ptr(light_positions), _ptr(light_intensities), _ptr(ambient),
                                        *tail, _ptr(ws), have, _stream(dev))
        else:
            need = L.mr_shade_backward_workspace_bytes(B, V, T, W, H)
            ws, have = _workspace(dev, need)
            rc = L.mr_shade_backward(_ptr(drgba), _ptr(ids), _ptr(bary), _ptr(clip), _ptr(normals),
                                     _ptr(positions), _ptr(diffuse), _ptr(triangles),
                                     _ptr(light_positions), _ptr(light_intensities), _ptr(ambient),
                                     *tail, _ptr(ws), have, _stream(dev))
    _check(rc, "mr_shade_backward")
    if lg is None:
        return dclip, dn, dp, dd, None, None, None
    dlpos = lg[:, :3 * nl].reshape(B, nl, 3)
    dlint = lg[:, 3 * nl:6 * nl].reshape(B, nl, 3)
    damb = lg[:, 6 * nl:] if ambient is not None else None
    return dclip, dn, dp, dd, dlpos, dlint, damb


def rasterize_specular_norms_forward(clip, triangles, normals, positions, light_positions, camera_position,
                                     width, height, want_z=False):
    """rasterize_forward(clip, triangles, width, height) AND the specular term's across-pixels norms in one pass over
    the pixels -> (ids, bary, z or None, norms2 [B,L]); 1 <= L <= shade_fast_lights().  norms2 goes to
    shade_specular_forward(..., norms2=) -- its norm pass over the G-buffer then does not run -- and to
    shade_specular_backward as before."""
    B, V, T = _chk_mesh(clip, triangles)
    for name, t in (("normals", normals), ("positions", positions)):
        _chk(name, t, _F32, B, V, 3)
    _chk("light_positions", light_positions, _F32, B, None, 3)
    nl = light_positions.shape[1]
    if not 1 <= nl <= shade_fast_lights():
        raise ValueError("1..%d lights per call" % shade_fast_lights())
    _chk("camera_position", camera_position, _F32, B, 3)
    dev = _require_device(clip, triangles, normals, positions, light_positions, camera_position)
    clip, triangles, normals, positions, light_positions, camera_position = [
        t.contiguous() for t in (clip, triangles, normals, positions, light_positions, camera_position)]
    width, height = int(width), int(height)
    ids = torch.empty(B, height, width, dtype=torch.int32, device=dev)
    bary = torch.empty(B, height, width, 3, dtype=torch.float32, device=dev)
    z = torch.empty(B, height, width, dtype=torch.float32, device=dev)
    norms2 = torch.empty(B, nl, dtype=torch.float32, device=dev)
    L = lib()
    with torch.cuda.device(dev):
        need = L.mr_rasterize_specular_norms_workspace_bytes(B, V, T, width, height)
        ws, have = _workspace(dev, need)
        rc = L.mr_rasterize_specular_norms_forward(
            _ptr(clip), _ptr(triangles), _ptr(normals), _ptr(positions), _ptr(light_positions), _ptr(camera_position),
            B, V, T, width, height, nl, _ptr(ids), _ptr(bary), _ptr(z), int(bool(want_z)), _ptr(norms2), _ptr(ws), have,
            _stream(dev))
    _check(rc, "mr_rasterize_specular_norms_forward")
    return ids, bary, (z if want_z else None), norms2


def shade_specular_forward(ids, bary, normals, positions, diffuse, specular, triangles, light_positions,
                           light_intensities, ambient, camera_position, shininess, norms2=None):
    """Fused interpolation + Phong with the specular term -> (rgba [B,H,W,4], norms2 [B,L]).
    shininess: [B] (one exponent per image) or [B,V] (per vertex).
    norms2 ([B,L], rasterize_specular_norms_forward's for the same G-buffer, normals, positions, lights and camera):
    given, the norm pass does not run and the same tensor is returned."""
    tensors = [ids, bary, normals, positions, diffuse, specular, triangles, light_positions,
               light_intensities, camera_position, shininess]
    _chk("triangles", triangles, _I32, None, 3)
    _chk("positions", positions, _F32, None, None, 3)
    B, V = positions.shape[0], positions.shape[1]
    for name, t in (("normals", normals), ("diffuse colors", diffuse), ("specular colors", specular)):
        _chk(name, t, _F32, B, V, 3)
    _chk_gbuffer(ids, bary, B)
    _chk_lights(light_positions, light_intensities, ambient, B, shade_fast_lights())
    _chk("camera_position", camera_position, _F32, B, 3)
    per_vertex = _chk_shininess(shininess, B, V)
    dev = _require_device(*(tensors + ([ambient] if ambient is not None else [])))
    L = lib()
    (ids, bary, normals, positions, diffuse, specular, triangles, light_positions, light_intensities,
     camera_position, shininess) = [t.contiguous() for t in tensors]
    ambient = ambient.contiguous() if ambient is not None else None
    B, H, W = ids.shape
    V, T, nl = normals.shape[1], triangles.shape[0], light_positions.shape[1]
    rgba = torch.empty(B, H, W, 4, dtype=torch.float32, device=dev)
    given = norms2 is not None
    if given:
        _chk("norms2", norms2, _F32, B, nl)
        _require_device(norms2)
        norms2 = norms2.contiguous()
    else:
        norms2 = torch.empty(B, nl, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        need = L.mr_shade_specular_forward_workspace_bytes(B, V, T, W, H)
        ws, have = _workspace(dev, need)
        rc = L.mr_shade_specular_forward(
            _ptr(ids), _ptr(bary), _ptr(normals), _ptr(positions), _ptr(diffuse), _ptr(specular),
            _ptr(triangles), _ptr(light_positions), _ptr(light_intensities), _ptr(ambient),
            _ptr(camera_position), _ptr(shininess), int(per_vertex), B, V, T, W, H, nl, _ptr(rgba),
            _ptr(norms2), int(given), _ptr(ws), have, _stream(dev))
    _check(rc, "mr_shade_specular_forward")
    return rgba, norms2


# grads_wanted bits of shade_specular_backward (include/mesh_raster.h: MR_GRAD_*)
GRAD_NORMALS, GRAD_POSITIONS, GRAD_DIFFUSE, GRAD_SPECULAR, GRAD_SHININESS, GRAD_LIGHTS, GRAD_CLIP = 1, 2, 4, 8, 16, 32, 64
GRAD_ALL = 127


def shade_specular_backward(drgba, ids, bary, clip, normals, positions, diffuse, specular, triangles,
                            light_positions, light_intensities, ambient, camera_position, shininess,
                            norms2, adjacency=None, transforms=None, normalised_gbuffer=False,
                            grads_wanted=GRAD_ALL, l1_signs=None):
    """-> (dclip [B,V,4], dnormals, dpositions, ddiffuse, dspecular [B,V,3], dlight_positions,
    dlight_intensities [B,L,3], dambient [B,3] or None, dcamera_position [B,3], dshininess shaped
    like shininess ([B] or [B,V])).  adjacency: vertex_adjacency(triangles, V) -- the per-triangle
    sums are then gathered per vertex (no atomics; required by the deterministic mode).

    grads_wanted: GRAD_* bits of the results the caller will read (the others come back unspecified).  With only
    GRAD_POSITIONS / GRAD_CLIP wanted and normalised_gbuffer=True (ids / bary are rasterize_forward's own output
    for `clip`) the pixel pass is the lane-accumulating kernel; with transforms ([B,4,4], clip = M (position, 1))
    and GRAD_CLIP not wanted, dpositions is the whole gradient w.r.t. the world-space vertices.

    l1_signs ([B,H,W] uint8, l1_loss_forward's sign codes for the image these inputs shaded): drgba is then the
    device scalar d L / d loss and the upstream image is upstream * sign / (B*H*W*4) without being written out where
    the pixel kernel can read the codes (mr_shade_specular_backward_l1)."""
    tensors = [drgba, ids, bary, clip, normals, positions, diffuse, specular, triangles,
               light_positions, light_intensities, camera_position, shininess, norms2]
    B, V, _ = _chk_mesh(clip, triangles)
    for name, t in (("normals", normals), ("positions", positions), ("diffuse colors", diffuse),
                    ("specular colors", specular)):
        _chk(name, t, _F32, B, V, 3)
    h, w = _chk_gbuffer(ids, bary, B)
    nl_ = _chk_lights(light_positions, light_intensities, ambient, B, shade_fast_lights())
    if l1_signs is None:
        _chk("upstream gradient", drgba, _F32, B, h, w, 4)
    else:
        if drgba.dtype != torch.float32 or drgba.numel() != 1:
            raise ValueError("with l1_signs the upstream gradient is one float32 (d L / d loss)")
        if l1_signs.dtype != torch.uint8 or l1_signs.numel() != B * h * w:
            raise ValueError("l1_signs must hold one byte per pixel")
        _require_device(l1_signs)
        l1_signs = l1_signs.contiguous()
    _chk("camera_position", camera_position, _F32, B, 3)
    per_vertex = _chk_shininess(shininess, B, V)
    _chk("norms2", norms2, _F32, B, nl_)
    dev = _require_device(*(tensors + ([ambient] if ambient is not None else [])))
    L = lib()
    (drgba, ids, bary, clip, normals, positions, diffuse, specular, triangles, light_positions,
     light_intensities, camera_position, shininess, norms2) = [t.contiguous() for t in tensors]
    ambient = ambient.contiguous() if ambient is not None else None
    B, H, W = ids.shape
    V, T, nl = normals.shape[1], triangles.shape[0], light_positions.shape[1]
    dclip = torch.empty(B, V, 4, dtype=torch.float32, device=dev)
    dn, dp, dd, dsp = [torch.empty(B, V, 3, dtype=torch.float32, device=dev) for _ in range(4)]
    lg = torch.empty(B, 6 * nl + 7, dtype=torch.float32, device=dev)
    dshin_v = torch.empty(B, V, dtype=torch.float32, device=dev) if per_vertex else None
    if adjacency is not None:
        _chk("adjacency offsets", adjacency[0], _I32, V + 1)
        _chk("adjacency entries", adjacency[1], _I32, None)
    if transforms is not None:
        _chk("transforms", transforms, _F32, B, 4, 4)
        _require_device(transforms)
        transforms = transforms.contiguous()
    with torch.cuda.device(dev):
        _sync_deterministic()
        if l1_signs is not None:
            need = L.mr_shade_specular_backward_l1_workspace_bytes(B, V, T, W, H)
            entry, head = L.mr_shade_specular_backward_l1, (_ptr(l1_signs), _ptr(drgba))
        else:
            need = L.mr_shade_specular_backward_workspace_bytes(B, V, T, W, H)
            entry, head = L.mr_shade_specular_backward, (_ptr(drgba),)
        ws, have = _workspace(dev, need)
        rc = entry(
            *head, _ptr(ids), _ptr(bary), _ptr(clip), _ptr(normals), _ptr(positions),
            _ptr(diffuse), _ptr(specular), _ptr(triangles), _ptr(light_positions),
            _ptr(light_intensities), _ptr(ambient), _ptr(camera_position), _ptr(shininess),
            int(per_vertex), _ptr(norms2), B, V, T, W, H, nl, _ptr(dclip), _ptr(dn), _ptr(dp), _ptr(dd),
            _ptr(dsp), _ptr(dshin_v), _ptr(lg), _ptr(adjacency[0]) if adjacency is not None else None,
            _ptr(adjacency[1]) if adjacency is not None else None, _ptr(transforms),
            GBUFFER_NORMALISED if normalised_gbuffer else 0, int(grads_wanted), _ptr(ws), have, _stream(dev))
    _check(rc, "mr_shade_specular_backward_l1" if l1_signs is not None else "mr_shade_specular_backward")
    dlpos = lg[:, :3 * nl].reshape(B, nl, 3)
    dlint = lg[:, 3 * nl:6 * nl].reshape(B, nl, 3)
    damb = lg[:, 6 * nl:6 * nl + 3] if ambient is not None else None
    dcam = lg[:, 6 * nl + 3:6 * nl + 6]
    dshin = dshin_v if per_vertex else lg[:, 6 * nl + 6]
    return dclip, dn, dp, dd, dsp, dlpos, dlint, damb, dcam, dshin


def soft_max_lights():
    return int(lib().mr_soft_max_lights())


def soft_forward(clip, positions, normals, diffuse, triangles, light_positions, light_intensities,
                 width, height, sigma, gamma, blur, keep_prepared=False):
    """SoftRas forward: -> (rgba [B,H,W,4] with row 0 = top, aux [B,H,W,4] for the backward).

    keep_prepared=True runs in a workspace of its own and returns it as a third value: handed to
    soft_backward(prepared=...) for the same inputs, the per-triangle records and candidate lists the
    forward built there are not built again."""
    tensors = [clip, positions, normals, diffuse, triangles, light_positions, light_intensities]
    B, V, _ = _chk_mesh(clip, triangles)
    for name, t in (("positions", positions), ("normals", normals), ("diffuse colors", diffuse)):
        _chk(name, t, _F32, B, V, 3)
    _chk("light_positions", light_positions, _F32, B, None, 3)
    _chk("light_intensities", light_intensities, _F32, B, light_positions.shape[1])
    if not 1 <= light_positions.shape[1] <= soft_max_lights():
        raise ValueError("the soft rasterizer supports 1..%d lights" % soft_max_lights())
    dev = _require_device(*tensors)
    L = lib()
    clip, positions, normals, diffuse, triangles, light_positions, light_intensities = [
        t.contiguous() for t in tensors]
    B, V, _ = clip.shape
    T, nl = triangles.shape[0], light_positions.shape[1]
    rgba = torch.empty(B, height, width, 4, dtype=torch.float32, device=dev)
    aux = torch.empty(B, height, width, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        need = L.mr_soft_workspace_bytes(B, V, T, width, height)
        if keep_prepared:
            ws = torch.empty(max(int(L.mr_soft_prepared_bytes(B, V, T, width, height)), 256),
                             dtype=torch.uint8, device=dev)
            have = ws.numel()
        else:
            ws, have = _workspace(dev, need)
        rc = L.mr_soft_forward(_ptr(clip), _ptr(positions), _ptr(normals), _ptr(diffuse), _ptr(triangles),
                               _ptr(light_positions), _ptr(light_intensities), B, V, T, width, height, nl,
                               float(sigma), float(gamma), float(blur), _ptr(rgba), _ptr(aux), _ptr(ws),
                               have, _stream(dev))
    _check(rc, "mr_soft_forward")
    if keep_prepared:
        return rgba, aux, ws
    return rgba, aux


def soft_backward(drgba, rgba, aux, clip, positions, normals, diffuse, triangles, light_positions,
                  light_intensities, sigma, gamma, blur, prepared=None):
    """-> (dclip [B,V,4], dpositions, dnormals, ddiffuse [B,V,3], dlight_positions [B,L,3],
    dlight_intensities [B,L]).  prepared: the third value of soft_forward(keep_prepared=True) for the
    same inputs, or None."""
    tensors = [drgba, rgba, aux, clip, positions, normals, diffuse, triangles, light_positions,
               light_intensities]
    B, V, _ = _chk_mesh(clip, triangles)
    for name, t in (("positions", positions), ("normals", normals), ("diffuse colors", diffuse)):
        _chk(name, t, _F32, B, V, 3)
    _chk("light_positions", light_positions, _F32, B, None, 3)
    _chk("light_intensities", light_intensities, _F32, B, light_positions.shape[1])
    _chk("rgba", rgba, _F32, B, None, None, 4)
    _chk("aux", aux, _F32, B, rgba.shape[1], rgba.shape[2], 4)
    _chk("upstream gradient", drgba, _F32, B, rgba.shape[1], rgba.shape[2], 4)
    dev = _require_device(*tensors)
    L = lib()
    (drgba, rgba, aux, clip, positions, normals, diffuse, triangles, light_positions,
     light_intensities) = [t.contiguous() for t in tensors]
    B, V, _ = clip.shape
    T, nl = triangles.shape[0], light_positions.shape[1]
    _, H, W, _ = rgba.shape
    # one allocation, laid out back to back (dclip, dpositions, dnormals, ddiffuse, dlight_positions,
    # dlight_intensities): the library then zeroes all six with one memset instead of six launches
    n4, n3, nl3 = B * V * 4, B * V * 3, B * nl * 3
    flat = torch.empty(n4 + 3 * n3 + nl3 + B * nl, dtype=torch.float32, device=dev)
    dclip = flat[:n4].view(B, V, 4)
    dp = flat[n4:n4 + n3].view(B, V, 3)
    dn = flat[n4 + n3:n4 + 2 * n3].view(B, V, 3)
    dd = flat[n4 + 2 * n3:n4 + 3 * n3].view(B, V, 3)
    dlp = flat[n4 + 3 * n3:n4 + 3 * n3 + nl3].view(B, nl, 3)
    dli = flat[n4 + 3 * n3 + nl3:].view(B, nl)
    with torch.cuda.device(dev):
        _sync_deterministic()
        if prepared is not None and (prepared.device != dev or prepared.dtype != torch.uint8 or
                                     prepared.numel() < L.mr_soft_prepared_bytes(B, V, T, W, H)):
            raise ValueError("prepared must be the workspace soft_forward(keep_prepared=True) returned "
                             "for these sizes")
        need = L.mr_soft_workspace_bytes(B, V, T, W, H)
        ws, have = _workspace(dev, need)
        rc = L.mr_soft_backward(_ptr(drgba), _ptr(rgba), _ptr(aux), _ptr(clip), _ptr(positions),
                                _ptr(normals), _ptr(diffuse), _ptr(triangles), _ptr(light_positions),
                                _ptr(light_intensities), B, V, T, W, H, nl, float(sigma), float(gamma),
                                float(blur), _ptr(dclip), _ptr(dp), _ptr(dn), _ptr(dd), _ptr(dlp),
                                _ptr(dli), _ptr(prepared) if prepared is not None else None, _ptr(ws), have,
                                _stream(dev))
    _check(rc, "mr_soft_backward")
    return dclip, dp, dn, dd, dlp, dli


def image_empty_regions(image, out=None):
    """[B, ceil(H/64), ceil(W/64)] uint8 map of a [B,H,W,4] float32 device image: 1 = the 64 x 64 block (counted in
    G-buffer rows, i.e. from the image's LAST row up) is whole and all zeros.  What render_forward writes for its own
    image; l1_loss_forward skips blocks that are empty on both sides.  out: a map of that shape to overwrite in place."""
    _chk("image", image, _F32, None, None, None, 4)
    dev = _require_device(image)
    image = image.contiguous()
    B, H, W = image.shape[:3]
    if out is None:
        out = torch.empty(B, (H + 63) // 64, (W + 63) // 64, dtype=torch.uint8, device=dev)
    else:
        _chk("out", out, _U8, B, (H + 63) // 64, (W + 63) // 64)
        _require_device(image, out)
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
    with torch.cuda.device(dev):
        rc = lib().mr_image_empty_regions(_ptr(image), B, H, W, _ptr(out), _stream(dev))
    _check(rc, "mr_image_empty_regions")
    return out


def l1_loss_forward(a, b, want_signs=True, empty_a=None, empty_b=None):
    """mean |a - b| over all elements -> (0-D tensor, packed signs or None), on the device.

    The signs ((n + 3) // 4 bytes, 2 bits per element) are all the backward pass needs.

    empty_a, empty_b (both or neither; [B,H,W,4] images only): the images' empty-block maps (render_forward's
    want_empty_regions / image_empty_regions): blocks empty on both sides are not read."""
    if a.dtype != _F32 or b.dtype != _F32:
        raise RuntimeError("l1_loss expects float32 tensors")
    if a.shape != b.shape:
        raise ValueError("image and target must have the same shape")
    dev = _require_device(a, b)
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty((), dtype=torch.float32, device=dev)
    signs = torch.empty((a.numel() + 3) // 4, dtype=torch.uint8, device=dev) if want_signs else None
    partials = torch.empty(lib().mr_l1_loss_partials(), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _arm_timer(TIMER_L1_FORWARD)
        if empty_a is not None and empty_b is not None:
            _chk("image", a, _F32, None, None, None, 4)
            B, H, W = a.shape[:3]
            for name, m in (("empty_a", empty_a), ("empty_b", empty_b)):
                _chk(name, m, _U8, B, (H + 63) // 64, (W + 63) // 64)
            rc = lib().mr_l1_loss_forward_regions(_ptr(a), _ptr(b), B, H, W, _ptr(empty_a.contiguous()),
                                                  _ptr(empty_b.contiguous()), _ptr(out),
                                                  _ptr(signs) if want_signs else None, _ptr(partials), _stream(dev))
        else:
            rc = lib().mr_l1_loss_forward(_ptr(a), _ptr(b), a.numel(), _ptr(out),
                                          _ptr(signs) if want_signs else None, _ptr(partials), _stream(dev))
    _check(rc, "mr_l1_loss_forward")
    return out, signs


def l1_loss_backward(signs, shape, upstream):
    """upstream * sign(a - b) / n as a float32 tensor of `shape`, from the packed signs."""
    _chk("signs", signs, _U8, None)
    _chk("upstream gradient of the loss", upstream, _F32, 1)
    dev = _require_device(signs, upstream)
    da = torch.empty(shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib().mr_l1_loss_backward(_ptr(signs), da.numel(), _ptr(upstream.contiguous()), _ptr(da),
                                       _stream(dev))
    _check(rc, "mr_l1_loss_backward")
    return da


SSIM_SAME, SSIM_VALID = 0, 1                # mesh_raster.h, MR_SSIM_*
SSIM_GRAD_IMAGE, SSIM_GRAD_TARGET = 1, 2
_SSIM_PADDING = {"same": SSIM_SAME, "valid": SSIM_VALID}


def _chk_ssim(image, target, window_size, sigma, padding):
    """The argument rules of mr_ssim_forward / _backward -> (B, H, W, C, padding code)."""
    if not torch.is_tensor(image) or not torch.is_tensor(target):
        raise TypeError("image and target must be tensors")
    if image.shape != target.shape:
        raise ValueError("image and target must have the same shape")
    if image.dim() != 4:
        raise ValueError("ssim expects [B, H, W, C] images, got shape %s" % (list(image.shape),))
    if image.dtype != _F32 or target.dtype != _F32:
        raise RuntimeError("ssim expects float32 tensors")
    B, H, W, C = image.shape
    if not 1 <= C <= 4:
        raise ValueError("ssim supports 1..4 channels, got %d" % C)
    if B < 1 or H < 1 or W < 1:
        raise ValueError("ssim needs at least one image of at least one pixel, got shape %s" % (list(image.shape),))
    if isinstance(window_size, bool) or not isinstance(window_size, int) or window_size % 2 == 0 or \
            not 3 <= window_size <= 11:
        raise ValueError("window_size must be an odd integer in [3, 11], got %r" % (window_size,))
    if not (float(sigma) > 0.0 and float(sigma) < float("inf")):
        raise ValueError("sigma must be positive and finite, got %r" % (sigma,))
    if padding not in _SSIM_PADDING:
        raise ValueError("padding must be 'same' or 'valid', got %r" % (padding,))
    if padding == "valid" and (H < window_size or W < window_size):
        raise ValueError("padding='valid' needs H, W >= window_size, got %d x %d for a window of %d"
                         % (H, W, window_size))
    return B, H, W, C, _SSIM_PADDING[padding]


def ssim_forward(image, target, window_size=11, sigma=1.5, padding="same", c1=1e-4, c2=9e-4, grads=0,
                 want_map=False):
    """Mean SSIM of two [B,H,W,C] float32 device images (mr_ssim_forward) -> (0-D tensor, map or None, saved or None).

    grads: mask of SSIM_GRAD_IMAGE | SSIM_GRAD_TARGET, the inputs ssim_backward will differentiate; `saved` is the
    block of derivative planes it needs (None for grads = 0).  want_map: also the [B,H',W',C] SSIM map."""
    B, H, W, C, pad = _chk_ssim(image, target, window_size, sigma, padding)
    if not (c1 > 0.0 and c2 > 0.0 and c1 < float("inf") and c2 < float("inf")):
        raise ValueError("c1 and c2 must be positive and finite, got %r, %r" % (c1, c2))
    if grads not in (0, 1, 2, 3):
        raise ValueError("grads must be a mask of SSIM_GRAD_IMAGE | SSIM_GRAD_TARGET, got %r" % (grads,))
    dev = _require_device(image, target)
    L = lib()
    image, target = image.contiguous(), target.contiguous()
    Hm, Wm = (H - window_size + 1, W - window_size + 1) if pad == SSIM_VALID else (H, W)
    out = torch.empty((), dtype=_F32, device=dev)
    ssim_map = torch.empty(B, Hm, Wm, C, dtype=_F32, device=dev) if want_map else None
    saved = torch.empty(L.mr_ssim_saved_floats(B, H, W, C, window_size, pad, grads), dtype=_F32, device=dev) \
        if grads else None
    partials = torch.empty(L.mr_ssim_partials(B, H, W, window_size, pad), dtype=_F32, device=dev)
    with torch.cuda.device(dev):
        rc = L.mr_ssim_forward(_ptr(image), _ptr(target), B, H, W, C, window_size, float(sigma), float(c1), float(c2),
                               pad, grads, _ptr(out), _ptr(ssim_map), _ptr(saved), _ptr(partials), _stream(dev))
    _check(rc, "mr_ssim_forward")
    return out, ssim_map, saved


def ssim_backward(image, target, saved, upstream, window_size=11, sigma=1.5, padding="same", grads=SSIM_GRAD_IMAGE,
                  want_image=True, want_target=False):
    """(d image, d target) of upstream * mean SSIM from ssim_forward's saved block (same window, padding and grads);
    a gradient that is not wanted is None and is not computed."""
    B, H, W, C, pad = _chk_ssim(image, target, window_size, sigma, padding)
    if grads not in (1, 2, 3):
        raise ValueError("grads must be a non-empty mask of SSIM_GRAD_IMAGE | SSIM_GRAD_TARGET, got %r" % (grads,))
    if (want_image and not grads & SSIM_GRAD_IMAGE) or (want_target and not grads & SSIM_GRAD_TARGET):
        raise ValueError("the forward call saved nothing for a gradient that is wanted now (grads = %d)" % grads)
    L = lib()
    _chk("saved", saved, _F32, L.mr_ssim_saved_floats(B, H, W, C, window_size, pad, grads))
    _chk("upstream gradient of the ssim value", upstream, _F32, 1)
    dev = _require_device(image, target, saved, upstream)
    image, target, saved = image.contiguous(), target.contiguous(), saved.contiguous()
    da = torch.empty(B, H, W, C, dtype=_F32, device=dev) if want_image else None
    db = torch.empty(B, H, W, C, dtype=_F32, device=dev) if want_target else None
    with torch.cuda.device(dev):
        rc = L.mr_ssim_backward(_ptr(image), _ptr(target), _ptr(saved), _ptr(upstream.contiguous()), B, H, W, C,
                                window_size, float(sigma), pad, grads, _ptr(da), _ptr(db), _stream(dev))
    _check(rc, "mr_ssim_backward")
    return da, db


def export_u8(image):
    """trunc(clamp(image, 0, 1) * 255) as a uint8 tensor of the same shape (device)."""
    dev = _require_device(image)
    image = image.contiguous()
    out = torch.empty(image.shape, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib().mr_export_u8(_ptr(image), image.numel(), _ptr(out), _stream(dev))
    _check(rc, "mr_export_u8")
    return out


def tone_map(image, gamma, as_uint8=False):
    """tone_mapper of the reference on the device: clamp(image ** gamma / per-image max, 0, 1) for a
    [B, ...] float32 image -> float32 tensor of the same shape, or uint8 frames (as_uint8)."""
    if not torch.is_tensor(image) or image.dim() < 1:
        raise ValueError("image must be a [batch, ...] tensor")
    _chk("image", image, _F32, *([None] * image.dim()))
    dev = _require_device(image)
    image = image.contiguous()
    B = image.shape[0]
    per_image = image.numel() // B if B else 0
    scratch = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
    out = torch.empty(image.shape, dtype=torch.uint8 if as_uint8 else torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib().mr_tone_map(_ptr(image), B, per_image, float(gamma), _ptr(scratch),
                               None if as_uint8 else _ptr(out), _ptr(out) if as_uint8 else None, _stream(dev))
    _check(rc, "mr_tone_map")
    return out


def vertex_normals_forward(vertices, triangles, adjacency=None):
    """-> (normals [B,V,3], sums [B,V,3]); compute_vertex_normals of the reference as a per-vertex gather.
    adjacency: vertex_adjacency(triangles, V) if the caller already holds it."""
    _chk("vertices", vertices, _F32, None, None, 3)
    _chk("triangles", triangles, _I32, None, 3)
    dev = _require_device(vertices, triangles)
    vertices, triangles = vertices.contiguous(), triangles.contiguous()
    B, V, _ = vertices.shape
    offsets, entries = adjacency if adjacency is not None else vertex_adjacency(triangles, V)
    sums, normals = torch.empty_like(vertices), torch.empty_like(vertices)
    with torch.cuda.device(dev):
        rc = lib().mr_vertex_normals_forward(_ptr(vertices), _ptr(triangles), _ptr(offsets), _ptr(entries), B, V,
                                             triangles.shape[0], _ptr(sums), _ptr(normals), _stream(dev))
    _check(rc, "mr_vertex_normals_forward")
    return normals, sums


def vertex_normals_backward(dnormals, vertices, sums, triangles, adjacency=None):
    """-> dvertices [B,V,3]."""
    _chk("vertices", vertices, _F32, None, None, 3)
    B, V, _ = vertices.shape
    _chk("dnormals", dnormals, _F32, B, V, 3)
    _chk("sums", sums, _F32, B, V, 3)
    _chk("triangles", triangles, _I32, None, 3)
    dev = _require_device(dnormals, vertices, sums, triangles)
    dnormals, vertices, sums, triangles = [t.contiguous() for t in (dnormals, vertices, sums, triangles)]
    offsets, entries = adjacency if adjacency is not None else vertex_adjacency(triangles, V)
    dvertices = torch.empty_like(vertices)
    with torch.cuda.device(dev):
        rc = lib().mr_vertex_normals_backward(_ptr(dnormals), _ptr(vertices), _ptr(sums), _ptr(triangles),
                                              _ptr(offsets), _ptr(entries), B, V, triangles.shape[0],
                                              _ptr(dvertices), _stream(dev))
    _check(rc, "mr_vertex_normals_backward")
    return dvertices


def _chk_cameras(eye, center, up, fov_y, near_clip, far_clip):
    _chk("camera position", eye, _F32, None, 3)
    B = eye.shape[0]
    _chk("camera lookat", center, _F32, B, 3)
    _chk("camera up", up, _F32, B, 3)
    for name, t in (("fov_y", fov_y), ("near_clip", near_clip), ("far_clip", far_clip)):
        _chk(name, t, _F32, B)
    return B


def camera_transforms(eye, center, up, fov_y, near_clip, far_clip, aspect_ratio):
    """perspective . look_at per image as ONE launch -> (transforms [B,4,4], degenerate flags: a 1-element
    int32 device tensor, bit 0 = eye ~ center, bit 1 = up ~ gaze for some image)."""
    B = _chk_cameras(eye, center, up, fov_y, near_clip, far_clip)
    tensors = [t.contiguous() for t in (eye, center, up, fov_y, near_clip, far_clip)]
    dev = _require_device(*tensors)
    out = torch.empty(B, 4, 4, dtype=torch.float32, device=dev)
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib().mr_camera_transforms(*[_ptr(t) for t in tensors], float(aspect_ratio), B, _ptr(out), _ptr(flags),
                                        _stream(dev))
    _check(rc, "mr_camera_transforms")
    return out, flags


def camera_transforms_backward(dtransforms, eye, center, up, fov_y, near_clip, far_clip, aspect_ratio):
    """-> (deye, dcenter, dup) [B,3]."""
    B = _chk_cameras(eye, center, up, fov_y, near_clip, far_clip)
    _chk("gradient of the transforms", dtransforms, _F32, B, 4, 4)
    tensors = [t.contiguous() for t in (dtransforms, eye, center, up, fov_y, near_clip, far_clip)]
    dev = _require_device(*tensors)
    outs = [torch.empty(B, 3, dtype=torch.float32, device=dev) for _ in range(3)]
    with torch.cuda.device(dev):
        rc = lib().mr_camera_transforms_backward(*[_ptr(t) for t in tensors], float(aspect_ratio), B,
                                                 *[_ptr(t) for t in outs], _stream(dev))
    _check(rc, "mr_camera_transforms_backward")
    return tuple(outs)
