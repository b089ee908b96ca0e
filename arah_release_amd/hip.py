"""ctypes binding of the C ABI in include/arah_hip.h (libarah_hip.so, built by __graft_entry__.build()).

Only raw device pointers, sizes and the current HIP stream cross the boundary; torch is used for
device memory and streams.  There is NO fallback: if the shared library is missing or no GPU is
present, every entry point raises.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# ARAH_LIB_PATH: load another build of the same ABI (the instrumented one of tools/phase_clocks.py)
LIB_PATH = os.environ.get("ARAH_LIB_PATH") or os.path.join(_HERE, "libarah_hip.so")

ARAH_MAX_STEPS = 128
COLOR_NO_VIEW_DIR = 0
COLOR_IDR = 1
PRECISION_SPLIT_F16 = 0   # fp32 carried as hi + lo f16 pairs on the f16 matrix pipe (default)
PRECISION_FP32 = 1        # v_mfma_f32_16x16x4_f32 everywhere


SHADE_ENGINE_DEFAULT, SHADE_ENGINE_FP32 = 0, 1
CANON_KERNEL_WAVE, CANON_KERNEL_TILE, CANON_KERNEL_WAVE_L2 = 0, 1, 2


def default_shade_engine():
    """ARAH_SHADE_ENGINE=fp32: loop D's normal sweep and colour MLP on the fp32 MFMA; default bf16 x 3 (split frames)."""
    return SHADE_ENGINE_FP32 if os.environ.get("ARAH_SHADE_ENGINE", "b3") == "fp32" else SHADE_ENGINE_DEFAULT


def default_canon_kernel():
    """ARAH_CANON_KERNEL = wave (default) | tile | wave_l2: loop C's solver on split-engine frames."""
    return {"tile": CANON_KERNEL_TILE, "wave_l2": CANON_KERNEL_WAVE_L2}.get(os.environ.get("ARAH_CANON_KERNEL", "wave"), CANON_KERNEL_WAVE)


def default_precision():
    """ARAH_PRECISION=fp32 selects the exact engine for every GEMM; default is the split engine."""
    v = os.environ.get("ARAH_PRECISION", "split").lower()
    if v in ("split", "split_f16", "f16x3", "0"):
        return PRECISION_SPLIT_F16
    if v in ("fp32", "f32", "exact", "1"):
        return PRECISION_FP32
    raise ValueError("ARAH_PRECISION must be 'split' or 'fp32', got %r" % v)

_ERRORS = {-1: "ARAH_E_BADARG", -2: "ARAH_E_SHAPE", -3: "ARAH_E_WORKSPACE", -4: "ARAH_E_LAUNCH",
           -5: "ARAH_E_SAMPLING", -6: "ARAH_E_OVERFLOW"}

_fp = C.c_void_p  # device float*


class ArahNets(C.Structure):
    _fields_ = [("sdf_w", _fp * 7), ("sdf_b", _fp * 7), ("film_freq", _fp), ("film_phase", _fp),
                ("skin_w", _fp * 5), ("skin_b", _fp * 5), ("col_w", _fp * 6), ("col_b", _fp * 6),
                ("pose_vec", _fp), ("col_mode", C.c_int32), ("n_pose", C.c_int32), ("beta", _fp),
                ("precision", C.c_int32)]


class ArahBody(C.Structure):
    _fields_ = [("verts", _fp), ("vert_weights", _fp), ("bones", _fp), ("trans", _fp), ("center", _fp),
                ("coord_min", _fp), ("coord_max", _fp), ("n_verts", C.c_int32), ("prepared", C.c_void_p)]


class ArahSampling(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("n_near", C.c_int32), ("n_far", C.c_int32),
                ("cano_view_dirs", C.c_int32), ("render_last_pt", C.c_int32), ("full_shading", C.c_int32),
                ("lin_steps", _fp), ("lin_near", _fp), ("lin_far", _fp),
                ("shade_engine", C.c_int32), ("canon_kernel", C.c_int32),
                ("ev_canon", C.c_void_p * 2), ("ev_density", C.c_void_p * 2), ("ev_shade", C.c_void_p * 2),
                ("occupancy", C.c_void_p), ("ev_canon2", C.c_void_p * 2), ("ev_density2", C.c_void_p * 2)]


class ArahFrame(C.Structure):
    _fields_ = [("sdf_w0", _fp), ("sdf_wp", _fp * 5), ("sdf_wpT", _fp * 5), ("sdf_w6", _fp), ("sdf_b6", _fp),
                ("sdf_bias", _fp), ("sdf_freq", _fp), ("sdf_phase", _fp),
                ("sdf_wps", _fp * 5), ("sdf_fw", _fp), ("sdf_pw", _fp), ("sdf_fws", _fp),
                ("skin_w0", _fp), ("skin_wp", _fp * 3), ("skin_w4p", _fp), ("skin_bias", _fp),
                ("skin_wps", _fp * 4), ("skin_scales", _fp), ("skin_wpr", _fp), ("skin_wconsts", _fp),
                ("col_w0p", _fp), ("col_w1p", _fp), ("col_w2p", _fp), ("col_w3ap", _fp), ("col_w3bp", _fp),
                ("col_w4p", _fp), ("col_w5", _fp), ("col_bias", _fp),
                ("col_w0pT", _fp), ("col_w1pT", _fp), ("col_w2pT", _fp), ("col_w3apT", _fp), ("col_w3bpT", _fp),
                ("col_w4pT", _fp), ("b3", C.c_void_p * 22),
                ("verts4", _fp), ("knn_spheres", _fp), ("knn_grid", _fp), ("knn_cells", _fp),
                ("verts", _fp), ("vert_T", _fp), ("bones", _fp),
                ("scalars", _fp), ("n_verts", C.c_int32),
                ("col_mode", C.c_int32), ("precision", C.c_int32)]


class ArahTrainIn(C.Structure):
    _fields_ = [("n", C.c_int32), ("rotate_normal", C.c_int32), ("ray_augm", C.c_int32), ("geom_only", C.c_int32),
                ("x", _fp), ("T", _fp), ("view", _fp), ("view_orig", _fp), ("g_s", _fp), ("g_rgb", _fp),
                ("tap_cin", _fp), ("tap_c", _fp * 5), ("fwd_rgb4", _fp)]


class ArahTrainGrads(C.Structure):
    _fields_ = [("sdf", _fp), ("rgb4", _fp), ("gx4", _fp), ("film_freq", _fp), ("film_phase", _fp),
                ("h", _fp * 6), ("hd", _fp * 7), ("av", _fp * 6), ("avd", _fp * 6), ("cin", _fp), ("c", _fp * 5),
                ("d", _fp * 6)]


class ArahCounters(C.Structure):
    _fields_ = [("n_sdf_fwd", C.c_uint64), ("n_sdf_grad", C.c_uint64), ("n_skin_fwd", C.c_uint64),
                ("n_skin_jac", C.c_uint64), ("n_col", C.c_uint64), ("n_knn", C.c_uint64),
                ("n_density", C.c_uint64), ("n_canon", C.c_uint64), ("n_split_nonfinite", C.c_uint64),
                ("n_tier_rays", C.c_uint64), ("n_tier_rays_surface", C.c_uint64), ("n_tier_rays_promoted", C.c_uint64),
                ("n_tier_rays_skipped", C.c_uint64), ("n_tier_samples_p1", C.c_uint64), ("n_tier_samples_p2", C.c_uint64),
                ("n_tier_samples_skipped", C.c_uint64), ("n_tier_witnesses", C.c_uint64),
                ("n_tier_rays_untraced", C.c_uint64),
                ("n_canon_p2", C.c_uint64), ("n_density_p2", C.c_uint64)]


COUNTER_BYTES = C.sizeof(ArahCounters)
# the shading cull's two counters (n_shade_culled, n_shade_rescued) sit in the workspace directly behind ArahCounters
# (include/arah_hip.h: arah_shade_cull_counters)
CULL_COUNTER_BYTES = 16
SHADING_LAZY, SHADING_FULL, SHADING_LAZY_NO_CULL = 0, 1, 2   # ArahSampling.full_shading


class ArahTierAudit(C.Structure):
    _fields_ = [("a_examined", C.c_uint64), ("a_violations", C.c_uint64), ("b_examined", C.c_uint64),
                ("b_converged", C.c_uint64), ("b_violations", C.c_uint64), ("c_examined", C.c_uint64),
                ("c_violations", C.c_uint64), ("n_first", C.c_uint64), ("first_index", C.c_int64 * 8),
                ("first_class", C.c_int32 * 8), ("min_ratio", C.c_float), ("rate_log2", C.c_int32), ("seed", C.c_uint32),
                ("reserved", C.c_int32)]


AUDIT_BYTES = C.sizeof(ArahTierAudit)

EXPORTS = ["arah_frame_bytes", "arah_prepare_frame", "arah_body_bytes", "arah_prepare_body", "arah_workspace_bytes", "arah_counters_reset",
           "arah_counters_read", "arah_shade_cull_counters", "arah_sdf_eval", "arah_sdf_grid", "arah_rasterize", "arah_skin_lbs", "arah_skin_jacobian", "arah_color_eval",
           "arah_nearest_inverse_lbs", "arah_broyden3_lbs", "arah_joint_root_find", "arah_trace", "arah_sample_canonicalize",
           "arah_shade_composite", "arah_shade_points", "arah_render", "arah_shade_train_slab_bytes", "arah_shade_train_forward",
           "arah_shade_train_backward", "arah_composite_train_forward", "arah_composite_train_backward", "arah_gram_skinny_blocks", "arah_gram_skinny", "arah_colsum_blocks", "arah_colsum", "arah_inverse3x3", "arah_hsoftmax_train_forward", "arah_hsoftmax_train_backward", "arah_pose_tree_forward", "arah_pose_tree_backward", "arah_gemv_rows", "arah_mesh_query_scratch_bytes", "arah_mesh_query", "arah_dominant_kernel",
           "arah_skin_lbs_counted", "arah_marching_cubes_scratch_bytes", "arah_marching_cubes",
           "arah_marching_cubes_indexed_scratch_bytes", "arah_marching_cubes_indexed",
           "arah_occupancy_bytes", "arah_prepare_occupancy", "arah_occupancy_info", "arah_tier_debug", "arah_debug_samples",
           "arah_sample_depths_debug", "arah_cell_clusters_debug",
           "arah_sdf_grid_band_scratch_bytes", "arah_sdf_grid_band", "arah_tier_audit_bytes", "arah_tier_audit",
           "arah_tier_audit_debug", "arah_occupancy_clear_box", "arah_render_maps_bytes", "arah_render_maps",
           "arah_query_posed_bytes", "arah_query_posed", "arah_sdf_grid_posed_bytes", "arah_sdf_grid_posed",
           "arah_image_metrics_bytes", "arah_image_metrics",
           "arah_mesh_index_bytes", "arah_mesh_index_build", "arah_mesh_closest", "arah_surface_metrics_bytes", "arah_surface_metrics", "arah_face_area_cumsum",
           "arah_mesh_components_scratch_bytes", "arah_mesh_components", "arah_mesh_select_scratch_bytes", "arah_mesh_select",
           "arah_mesh_simplify_scratch_bytes", "arah_mesh_simplify",
           "arah_mesh_quadric_place_scratch_bytes", "arah_mesh_quadric_place",
           "arah_mesh_collapse_round_scratch_bytes", "arah_mesh_collapse_round", "arah_mesh_collapse_round_bounded",
           "arah_mesh_subdivide_round_scratch_bytes", "arah_mesh_subdivide_round",
           "arah_mesh_flip_round_scratch_bytes", "arah_mesh_flip_round",
           "arah_mesh_adjacency_scratch_bytes", "arah_mesh_adjacency", "arah_mesh_vertex_normals", "arah_mesh_smooth", "arah_mesh_tangential",
           "arah_mesh_cotangent", "arah_mesh_laplacian_apply", "arah_mesh_curvature", "arah_mesh_smooth_cotangent_scratch_bytes",
           "arah_mesh_smooth_cotangent", "arah_mesh_solve_scratch_bytes", "arah_mesh_solve_begin", "arah_mesh_solve_steps",
           "arah_mesh_orient_scratch_bytes", "arah_mesh_orient", "arah_mesh_boundary_loops_scratch_bytes",
           "arah_mesh_boundary_loops", "arah_mesh_fill_holes_scratch_bytes", "arah_mesh_fill_holes",
           "arah_mesh_rasterize", "arah_mesh_rasterize_debug", "arah_mesh_interpolate", "arah_mesh_raycast", "arah_mesh_raycast_debug",
           "arah_point_index_bytes", "arah_point_index_build", "arah_point_nearest", "arah_sample_scores_bytes", "arah_sample_scores",
           "arah_contains_index_bytes", "arah_contains_index_count", "arah_contains_index_fill", "arah_mesh_contains",
           "arah_mesh_contains_grid", "arah_mesh_sdf_grid_bytes", "arah_mesh_sdf_grid",
           "arah_winding_index_bytes", "arah_winding_index_count", "arah_winding_index_fill", "arah_mesh_winding",
           "arah_mesh_winding_grid", "arah_mesh_intersections_scratch_bytes", "arah_mesh_intersections"]

_lib = None


def load_library():
    """dlopen libarah_hip.so (after torch, so that it binds to the HIP runtime torch already loaded)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libarah_hip.so is not built (%s): run `python -c 'import __graft_entry__ as g; "
                           "g.build()'` -- there is no CPU fallback for the hot path" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.arah_frame_bytes.restype = C.c_size_t
    lib.arah_body_bytes.restype = C.c_size_t
    lib.arah_workspace_bytes.restype = C.c_size_t
    lib.arah_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.arah_dominant_kernel.restype = C.c_char_p
    lib.arah_shade_train_slab_bytes.restype = C.c_size_t
    lib.arah_mesh_query_scratch_bytes.restype = C.c_size_t
    lib.arah_marching_cubes_scratch_bytes.restype = C.c_size_t
    lib.arah_marching_cubes_scratch_bytes.argtypes = [C.c_int32]
    lib.arah_marching_cubes_indexed_scratch_bytes.restype = C.c_size_t
    lib.arah_marching_cubes_indexed_scratch_bytes.argtypes = [C.c_int32]
    lib.arah_occupancy_bytes.restype = C.c_size_t
    lib.arah_sdf_grid_band_scratch_bytes.restype = C.c_size_t
    lib.arah_colsum_blocks.argtypes = [C.c_int64]
    lib.arah_tier_audit_bytes.restype = C.c_size_t
    lib.arah_tier_audit_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.arah_render_maps_bytes.restype = C.c_size_t
    lib.arah_render_maps_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.arah_query_posed_bytes.restype = C.c_size_t
    lib.arah_query_posed_bytes.argtypes = [C.c_int32]
    lib.arah_sdf_grid_posed_bytes.restype = C.c_size_t
    lib.arah_sdf_grid_posed_bytes.argtypes = [C.c_int32]
    lib.arah_image_metrics_bytes.restype = C.c_size_t
    lib.arah_image_metrics_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.arah_mesh_index_bytes.restype = C.c_size_t
    lib.arah_mesh_index_bytes.argtypes = [C.c_int32]
    lib.arah_surface_metrics_bytes.restype = C.c_size_t
    lib.arah_surface_metrics_bytes.argtypes = [C.c_int32, C.c_int32]
    for name in ("arah_point_index_bytes", "arah_sample_scores_bytes"):
        getattr(lib, name).restype = C.c_size_t
        getattr(lib, name).argtypes = [C.c_int32]
    for name in ("arah_mesh_components_scratch_bytes", "arah_mesh_select_scratch_bytes", "arah_mesh_adjacency_scratch_bytes",
                 "arah_mesh_quadric_place_scratch_bytes", "arah_mesh_collapse_round_scratch_bytes",
                 "arah_mesh_subdivide_round_scratch_bytes", "arah_mesh_flip_round_scratch_bytes",
                 "arah_mesh_smooth_cotangent_scratch_bytes", "arah_mesh_solve_scratch_bytes",
                 "arah_mesh_orient_scratch_bytes", "arah_mesh_boundary_loops_scratch_bytes", "arah_mesh_fill_holes_scratch_bytes"):
        getattr(lib, name).restype = C.c_size_t
        getattr(lib, name).argtypes = [C.c_int64, C.c_int64]
    lib.arah_mesh_simplify_scratch_bytes.restype = C.c_size_t
    lib.arah_mesh_simplify_scratch_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    lib.arah_contains_index_bytes.restype = C.c_size_t
    lib.arah_contains_index_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.arah_mesh_sdf_grid_bytes.restype = C.c_size_t
    lib.arah_mesh_sdf_grid_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64]
    lib.arah_winding_index_bytes.restype = C.c_size_t
    lib.arah_winding_index_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.arah_mesh_intersections_scratch_bytes.restype = C.c_size_t
    lib.arah_mesh_intersections_scratch_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    for name in EXPORTS:
        getattr(lib, name)  # AttributeError if the symbol is missing
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s (%d)" % (what, _ERRORS.get(rc, "?"), rc))


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    return C.c_void_p(t.data_ptr())


def _f32(t):
    return t.detach().to(dtype=torch.float32).contiguous()


_call_device = [None]   # device of the C-ABI call in flight (set by _guarded / Frame.__init__)


def _stream(device=None):
    """Current HIP stream OF the call's device (not of whatever device happens to be current)."""
    device = device if device is not None else _call_device[0]
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _on_device:
    """Make `device` current for the duration of a C-ABI call: the kernels, memsets and copies behind the ABI are
    issued on the current device, torch's own guard does not reach through ctypes."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.guard = torch.cuda.device(self.device)

    def __enter__(self):
        self.guard.__enter__()
        self.prev = _call_device[0]
        _call_device[0] = self.device

    def __exit__(self, *exc):
        _call_device[0] = self.prev
        return self.guard.__exit__(*exc)


def _guarded(fn):
    """Wrapper for fn(frame, ws, ...): frame, workspace and every tensor argument must share one GPU, which
    becomes the current device (and supplies the stream) for the call."""
    import functools

    @functools.wraps(fn)
    def wrapper(frame, ws, *args, **kwargs):
        dev = frame.device
        if ws.device != dev:
            raise ValueError("workspace lives on %s, frame on %s" % (ws.device, dev))

        def check(v):
            if isinstance(v, torch.Tensor):
                if v.device != dev:
                    raise ValueError("argument on %s, frame on %s" % (v.device, dev))
            elif isinstance(v, (tuple, list)):
                for u in v:
                    check(u)
        for v in list(args) + list(kwargs.values()):
            check(v)
        with _on_device(dev):
            return fn(frame, ws, *args, **kwargs)
    return wrapper


def _same_device(*tensors):
    """All device buffers of one C-ABI call must live on one GPU; returns it."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError("device-resident tensor required")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError("buffers of one call live on different devices: %s vs %s" % (dev, t.device))
    return dev


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("arah_release_amd needs a HIP device (MI355X / gfx950); none is visible and there "
                           "is no CPU fallback")


class Workspace:
    """Caller-owned scratch of the C ABI (grows on demand, never shrinks)."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.buf = None
        self.occ = None   # occupancy bitmap of the frame this scratch is rendering (tiered eval forward)
        self.audit_buf = None   # scratch of arah_tier_audit (allocated by the first audit: about one more workspace)
        self.maps_buf = None    # per-sample normals of arah_render_maps (allocated by the first render with maps)

    def occupancy(self, frame):
        """arah_prepare_occupancy for `frame` on the current stream, into this scratch's own buffer (a scratch serves one
        stream: the bitmap of the previous frame is dead by stream order when the next one is built)."""
        lib = load_library()
        buf = self.ensure(1, 1)
        with torch.cuda.device(self.device):
            if self.occ is None:
                self.occ = torch.empty(int(lib.arah_occupancy_bytes()), dtype=torch.uint8, device=self.device)
            _check(lib.arah_prepare_occupancy(C.byref(frame.handle), _ptr(self.occ), C.c_size_t(self.occ.numel()), _ptr(buf),
                                              C.c_size_t(buf.numel()), _stream(self.device)), "arah_prepare_occupancy")
        return self.occ

    def occupancy_info(self):
        """Header of the last occupancy built here (synchronises the stream): dict of its geometry and counts."""
        import struct
        out = (C.c_int32 * 16)()
        with torch.cuda.device(self.device):
            _check(load_library().arah_occupancy_info(_ptr(self.occ), out, _stream(self.device)), "arah_occupancy_info")
        raw = bytes(out)
        f = struct.unpack("5f", raw[:20])
        i = struct.unpack("9i", raw[20:56])
        return {"origin": f[:3], "voxel": f[3], "dims": i[:3], "n_vox": i[3], "valid": i[4], "n_cells": i[5], "n_fine": i[6],
                "n_selected": i[7], "overflow": i[8], "band_m": struct.unpack("f", raw[56:60])[0],
                "lip_pose": struct.unpack("f", raw[60:64])[0]}

    def occupancy_clear_box(self, lo, hi):
        """Tests only: unmark the voxels of this scratch's occupancy whose centres lie in the posed-space box [lo, hi] (metres) and
        recompute its distance transform -- a certificate damaged on purpose (arah_occupancy_clear_box)."""
        lo3, hi3 = (C.c_float * 3)(*[float(v) for v in lo]), (C.c_float * 3)(*[float(v) for v in hi])
        with torch.cuda.device(self.device):
            _check(load_library().arah_occupancy_clear_box(_ptr(self.occ), lo3, hi3, _stream(self.device)), "arah_occupancy_clear_box")

    def audit_ensure(self, n_rays, n_steps):
        need = load_library().arah_tier_audit_bytes(int(n_rays), int(n_steps))
        if self.audit_buf is None or self.audit_buf.numel() < need:
            self.audit_buf = None
            with torch.cuda.device(self.device):
                self.audit_buf = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.audit_buf

    def maps_ensure(self, n_rays, n_steps):
        need = load_library().arah_render_maps_bytes(int(n_rays), int(n_steps))
        if self.maps_buf is None or self.maps_buf.numel() < need:
            self.maps_buf = None
            with torch.cuda.device(self.device):
                self.maps_buf = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.maps_buf

    def tier_audit_debug(self, n_rays, n_steps):
        """(sample_tag [N*S], ray_tag [N]) uint8 verdicts of the last arah_tier_audit on this scratch (include/arah_hip.h)."""
        st = torch.empty(n_rays * n_steps, dtype=torch.uint8, device=self.device)
        rt = torch.empty(n_rays, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _check(load_library().arah_tier_audit_debug(_ptr(self.audit_buf), C.c_size_t(self.audit_buf.numel()), C.c_int32(n_rays),
                                                        C.c_int32(n_steps), _ptr(st), _ptr(rt), _stream(self.device)),
                   "arah_tier_audit_debug")
        return st, rt

    def tier_debug(self, n_rays, n_steps):
        """(ray_tier, ray_sigma_pos) uint8 tensors of the last arah_render on this scratch."""
        tier = torch.empty(n_rays, dtype=torch.uint8, device=self.device)
        pos = torch.empty(n_rays, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _check(load_library().arah_tier_debug(_ptr(self.buf), C.c_size_t(self.buf.numel()), C.c_int32(n_rays), C.c_int32(n_steps),
                                                  _ptr(tier), _ptr(pos), _stream(self.device)), "arah_tier_debug")
        return tier, pos

    def debug_samples(self, n_rays, n_steps, which=("z", "pts", "T", "mask", "shaded", "state")):
        """Per-sample arrays of the last arah_render on this scratch: dict of the tensors named in `which`."""
        d, Q = self.device, n_rays * n_steps
        make = {"z": lambda: torch.empty(Q, device=d), "pts": lambda: torch.empty(Q, 3, device=d), "T": lambda: torch.empty(Q, 16, device=d),
                "mask": lambda: torch.empty(Q, dtype=torch.uint8, device=d), "shaded": lambda: torch.empty(Q, 4, device=d),
                "state": lambda: torch.empty(Q, dtype=torch.uint8, device=d)}
        out = {k: make[k]() for k in which}
        with torch.cuda.device(d):
            _check(load_library().arah_debug_samples(_ptr(self.buf), C.c_size_t(self.buf.numel()), C.c_int32(n_rays), C.c_int32(n_steps),
                                                     _ptr(out.get("z")), _ptr(out.get("pts")), _ptr(out.get("T")), _ptr(out.get("mask")),
                                                     _ptr(out.get("shaded")), _ptr(out.get("state")), _stream(d)), "arah_debug_samples")
        return out

    def ensure(self, n_rays, n_steps):
        need = load_library().arah_workspace_bytes(int(n_rays), int(n_steps))
        if self.buf is None or self.buf.numel() < need:
            old = self.buf
            with torch.cuda.device(self.device):
                self.buf = torch.empty(need, dtype=torch.uint8, device=self.device)
                if old is None:
                    _check(load_library().arah_counters_reset(_ptr(self.buf), _stream(self.device)),
                           "arah_counters_reset")
                else:   # the work counters sit at the head of the workspace: a grown buffer inherits them
                    self.buf[:COUNTER_BYTES + CULL_COUNTER_BYTES].copy_(old[:COUNTER_BYTES + CULL_COUNTER_BYTES])
        return self.buf

    def reset_counters(self):
        with torch.cuda.device(self.device):
            _check(load_library().arah_counters_reset(_ptr(self.buf), _stream(self.device)), "arah_counters_reset")

    def counters(self):
        out = ArahCounters()
        with torch.cuda.device(self.device):
            _check(load_library().arah_counters_read(_ptr(self.buf), C.byref(out), _stream(self.device)),
                   "arah_counters_read")
            cull = (C.c_uint64 * 2)()
            _check(load_library().arah_shade_cull_counters(_ptr(self.buf), cull, _stream(self.device)),
                   "arah_shade_cull_counters")
        res = {k: int(getattr(out, k)) for k, _ in ArahCounters._fields_}
        res["n_shade_culled"], res["n_shade_rescued"] = int(cull[0]), int(cull[1])
        return res


# The occupancy buffer's layout (csrc/tier.hpp: the constants kOcc*, kTierBand; csrc/arah_hip.hip: carve_occ hands the arrays out in
# this order, each starting on a 256-byte boundary like Carver::take).  tests/test_occupancy_spec.py reads both out of the source.
OCC_NC, OCC_F, OCC_L, OCC_MAX_CELLS, OCC_MAX_VOX, OCC_ALIGN, TIER_BAND = 49, 3, 1.5, 12288, 1 << 22, 256, 18.0
OCC_MAX_FINE = OCC_MAX_CELLS * OCC_F ** 3
OCC_INFO_WORDS = 16   # OccInfo: origin[3], v, inv_v (float) | dims[3], n_vox, valid, n_cells, n_fine, n_sel, overflow (int) | band_m, lip_pose (float)
OCC_FIELDS = (("info", torch.int32, (OCC_INFO_WORDS,)), ("bits", torch.int32, (OCC_MAX_VOX // 32,)), ("dist", torch.uint8, (OCC_MAX_VOX,)),
              ("csdf", torch.float32, (OCC_NC ** 3,)), ("cpts", torch.float32, (OCC_NC ** 3, 3)),
              ("cell_lip", torch.float32, (OCC_MAX_CELLS,)), ("cell_stretch", torch.float32, (OCC_MAX_CELLS,)),
              ("fnorm", torch.float32, (OCC_MAX_FINE, 3)), ("fsdf", torch.float32, (OCC_MAX_FINE,)), ("iota", torch.int32, (OCC_MAX_FINE,)),
              ("sel_raw", torch.float32, (OCC_MAX_FINE, 3)), ("sel_bar", torch.float32, (OCC_MAX_FINE, 3)),
              ("sel_idx", torch.int32, (OCC_MAX_FINE,)), ("sel_of", torch.int32, (OCC_MAX_FINE,)))


def occupancy_layout():
    """[(name, byte offset, byte length, dtype, shape)] of the occupancy buffer's arrays, and the buffer's size."""
    out, off = [], 0
    for name, dt, shape in OCC_FIELDS:
        off = (off + OCC_ALIGN - 1) // OCC_ALIGN * OCC_ALIGN
        nbytes = torch.empty(0, dtype=dt).element_size()
        for s in shape:
            nbytes *= s
        out.append((name, off, nbytes, dt, shape))
        off += nbytes
    return out, (off + OCC_ALIGN - 1) // OCC_ALIGN * OCC_ALIGN


def occupancy_view(occ):
    """Tests only: the arrays of an occupancy buffer (Workspace.occupancy) as typed views onto it, no copy -- dict name -> tensor in
    the order of OCC_FIELDS.  `info` is the header's 16 words as int32 (its float fields: .view(torch.float32)); `bits` holds voxel
    b in bit b & 31 of word b >> 5."""
    layout, total = occupancy_layout()
    if occ.dtype != torch.uint8 or occ.dim() != 1 or occ.numel() < total:
        raise ValueError("occupancy_view: a uint8 buffer of at least %d bytes" % total)
    return {name: occ[off:off + nbytes].view(dt).reshape(shape) for name, off, nbytes, dt, shape in layout}


_side_streams = {}


class BodyTables:
    """The nearest-vertex tables of one posed body (k-d clustered vertices, cluster spheres, per-cell candidate lists),
    built by arah_prepare_body on a SIDE stream: the 1.4 ms of a one-workgroup sort and a 512-workgroup pass then run next to
    whatever the caller's stream does in the meantime (the pose encoder and the hypernetwork: the posed vertices are
    known before them).  Frame(..., body_tables=...) orders the side stream before its own and keeps this object alive."""

    def __init__(self, verts):
        require_gpu()
        lib = load_library()
        dev = verts.device
        self.verts = _f32(verts)
        self.verts_version = self.verts._version
        if self.verts.dim() != 2 or self.verts.shape[1] != 3:
            raise ValueError("verts must be (V, 3)")
        cur = torch.cuda.current_stream(dev)
        side = _side_streams.get(dev.index)
        if side is None:
            side = _side_streams[dev.index] = torch.cuda.Stream(device=dev)
        with _on_device(dev):
            self.buf = torch.empty(int(lib.arah_body_bytes()), dtype=torch.uint8, device=dev)
            side.wait_stream(cur)                       # the vertices (and the recycled buffer) are the caller's stream's
            self.buf.record_stream(side)
            self.verts.record_stream(side)
            _check(lib.arah_prepare_body(_ptr(self.verts), C.c_int32(int(self.verts.shape[0])), _ptr(self.buf),
                                         C.c_size_t(self.buf.numel()), C.c_void_p(side.cuda_stream)), "arah_prepare_body")
            self.done = torch.cuda.Event()
            self.done.record(side)
        self.device = dev


class Frame:
    """Packed per-frame state on the device (MFMA-ordered weights, padded vertices)."""

    def __init__(self, sdf_layers, film_freq, film_phase, skin_layers, color_layers, color_mode, pose_vec, beta,
                 verts, vert_weights, bones, trans, center, coord_min, coord_max, precision=None, body_tables=None):
        require_gpu()
        lib = load_library()
        dev = verts.device
        keep = []  # tensors referenced by raw pointers must outlive the call

        def own(t):
            t = _f32(t)
            keep.append(t)
            return t

        def scalar_tensor(v, n):
            """Per-frame scalars (trans, center, coord_min/max, |variance|) stay on the device: tensors are used as
            they are (no .item() / .tolist(): those drain the stream); python numbers are uploaded."""
            if isinstance(v, torch.Tensor):
                return v.to(device=dev, dtype=torch.float32).reshape(-1)[:n]
            return torch.tensor(v, dtype=torch.float32, device=dev).reshape(-1)[:n]

        nets = ArahNets()
        if color_layers is None:   # tracer-only use: the colour MLP is never evaluated
            color_mode, pose_vec = COLOR_NO_VIEW_DIR, None
            dims = [(256, 262), (256, 256), (128, 256), (256, 390), (256, 256), (3, 256)]
            color_layers = [(torch.zeros(d, device=dev), torch.zeros(d[0], device=dev)) for d in dims]
        if len(sdf_layers) != 7 or len(skin_layers) != 5 or len(color_layers) != 6:
            raise ValueError("unsupported network depth (ARAH_E_SHAPE)")
        shapes_sdf = [(256, 3)] + [(256, 256)] * 5 + [(1, 256)]
        for i, (w, b) in enumerate(sdf_layers):
            if tuple(w.shape) != shapes_sdf[i]:
                raise ValueError("SDF layer %d has shape %s, expected %s" % (i, tuple(w.shape), shapes_sdf[i]))
            nets.sdf_w[i] = _ptr(own(w)).value
            nets.sdf_b[i] = _ptr(own(b)).value
        nets.film_freq = _ptr(own(film_freq.reshape(-1)))
        nets.film_phase = _ptr(own(film_phase.reshape(-1)))
        shapes_skin = [(128, 3)] + [(128, 128)] * 3 + [(25, 128)]
        for i, (w, b) in enumerate(skin_layers):
            if tuple(w.shape) != shapes_skin[i]:
                raise ValueError("skinning layer %d has shape %s, expected %s" % (i, tuple(w.shape), shapes_skin[i]))
            nets.skin_w[i] = _ptr(own(w)).value
            nets.skin_b[i] = _ptr(own(b)).value
        n_pose = 0 if pose_vec is None else int(pose_vec.numel())
        in_dim = (33 if color_mode == COLOR_IDR else 6) + 256 + n_pose
        shapes_col = [(256, in_dim), (256, 256), (128, 256), (256, in_dim + 128), (256, 256), (3, 256)]
        for i, (w, b) in enumerate(color_layers):
            if tuple(w.shape) != shapes_col[i]:
                raise ValueError("colour layer %d has shape %s, expected %s" % (i, tuple(w.shape), shapes_col[i]))
            nets.col_w[i] = _ptr(own(w)).value
            nets.col_b[i] = _ptr(own(b)).value
        nets.pose_vec = _ptr(own(pose_vec.reshape(-1))) if n_pose else None
        nets.col_mode = int(color_mode)
        nets.n_pose = n_pose
        nets.beta = _ptr(own(scalar_tensor(beta, 1)))
        nets.precision = default_precision() if precision is None else int(precision)
        self.precision = nets.precision
        body = ArahBody()
        self.verts, self.vert_weights, self.bones = own(verts), own(vert_weights), own(bones.reshape(24, 16))
        body.verts, body.vert_weights, body.bones = _ptr(self.verts), _ptr(self.vert_weights), _ptr(self.bones)
        body.trans, body.center = _ptr(own(scalar_tensor(trans, 3))), _ptr(own(scalar_tensor(center, 3)))
        body.coord_min, body.coord_max = _ptr(own(scalar_tensor(coord_min, 1))), _ptr(own(scalar_tensor(coord_max, 1)))
        body.n_verts = int(verts.shape[0])
        self.body_tables = body_tables
        if body_tables is not None:
            # the tables must be THESE vertices': same storage, untouched since (a reused inputs dict whose smpl_verts were
            # replaced or modified in place after the tables were built would otherwise be searched with a stale body)
            same = tuple(body_tables.verts.shape) == tuple(self.verts.shape) and (
                (body_tables.verts.data_ptr() == self.verts.data_ptr() and body_tables.verts_version == self.verts._version)
                or bool(torch.equal(body_tables.verts, self.verts)))
            if body_tables.device != dev or not same:
                raise ValueError("body_tables were built for another body / device")
            torch.cuda.current_stream(dev).wait_event(body_tables.done)
            body.prepared = body_tables.buf.data_ptr()
        _same_device(*keep)
        nbytes = lib.arah_frame_bytes(C.byref(nets), C.byref(body))
        self.handle = ArahFrame()
        with _on_device(dev):
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _check(lib.arah_prepare_frame(C.byref(nets), C.byref(body), _ptr(self.buf), C.c_size_t(nbytes),
                                          C.byref(self.handle), _stream()), "arah_prepare_frame")
        # the pack kernels read `keep` asynchronously on the current stream; hold the raw tensors
        # until the frame is dropped (cheap: a few MB)
        self._keep = keep
        self.device = dev
        self.color_mode = int(color_mode)


class Sampling:
    """ArahSampling + the device linspace tables (bit-identical to torch.linspace on the CPU)."""

    def __init__(self, device, n_steps=64, n_near=16, n_far=16, cano_view_dirs=True, render_last_pt=False,
                 full_shading=False, shade_engine=None, canon_kernel=None, shade_cull=True):
        if n_steps < n_near + n_far + 1 or n_steps > ARAH_MAX_STEPS:
            raise ValueError("need n_near + n_far + 1 <= n_steps <= %d (ARAH_E_SAMPLING)" % ARAH_MAX_STEPS)
        self.lin_steps = torch.linspace(0.0, 1.0, n_steps, dtype=torch.float32).to(device)
        self.lin_near = torch.linspace(0.0, 1.0, n_near + 1, dtype=torch.float32).to(device)
        self.lin_far = torch.linspace(0.0, 1.0, max(n_far, 1), dtype=torch.float32).to(device)
        s = ArahSampling()
        s.n_steps, s.n_near, s.n_far = int(n_steps), int(n_near), int(n_far)
        s.cano_view_dirs, s.render_last_pt = int(bool(cano_view_dirs)), int(bool(render_last_pt))
        # lazy shading also leaves the sigma > 0 samples unshaded whose weight cannot change a pixel (same image, bit for bit)
        # unless shade_cull is False
        s.full_shading = SHADING_FULL if full_shading else (SHADING_LAZY if shade_cull else SHADING_LAZY_NO_CULL)
        s.lin_steps, s.lin_near, s.lin_far = _ptr(self.lin_steps), _ptr(self.lin_near), _ptr(self.lin_far)
        # per-call switches of the library (it reads no environment itself): None = this process's default
        s.shade_engine = default_shade_engine() if shade_engine is None else int(shade_engine)
        s.canon_kernel = default_canon_kernel() if canon_kernel is None else int(canon_kernel)
        self.handle = s
        self._events = {}
        self.n_steps, self.n_near, self.n_far = n_steps, n_near, n_far

    def set_events(self, which, start=None, stop=None):
        """Profiling hook of THIS sampling object: every call that takes it records the torch.cuda.Event pair on its stream
        around loop C's solver ("canon"), the density pre-pass ("density") or the shading kernel ("shade").  None switches
        it off.  (Round 3 kept the handles in process-wide variables of the library.)"""
        field = getattr(self.handle, {"canon": "ev_canon", "density": "ev_density", "shade": "ev_shade", "canon2": "ev_canon2",
                                      "density2": "ev_density2"}[which])
        for ev in (start, stop):   # torch creates the hipEvent lazily, on the first record
            if ev is not None and not ev.cuda_event:
                ev.record()
        field[0] = start.cuda_event if start is not None else None
        field[1] = stop.cuda_event if stop is not None else None
        self._events[which] = (start, stop)   # keep them alive


# ------------------------------------------------------------------------------------------------
# thin functional wrappers (allocate outputs with torch, call the C ABI on the current stream)
# ------------------------------------------------------------------------------------------------
@_guarded
def sdf_eval(frame, ws, x_norm, want_feat=False, want_grad=False):
    lib = load_library()
    x = _f32(x_norm)
    n = x.shape[0]
    buf = ws.ensure(1, 1)
    sdf = torch.empty(n, device=x.device)
    feat = torch.empty(n, 256, device=x.device) if want_feat else None
    grad = torch.empty(n, 3, device=x.device) if want_grad else None
    _check(lib.arah_sdf_eval(C.byref(frame.handle), _ptr(x), C.c_int32(n), _ptr(sdf), _ptr(feat), _ptr(grad),
                             _ptr(buf), C.c_size_t(buf.numel()), _stream()), "arah_sdf_eval")
    return sdf, feat, grad


@_guarded
def sdf_grid(frame, ws, n_side=256):
    """SDF on the n_side^3 lattice of [-1,1]^3 -> (n_side, n_side, n_side) tensor [ix, iy, iz], on the device."""
    lib = load_library()
    buf = ws.ensure(1, 1)
    out = torch.empty(n_side, n_side, n_side, device=frame.device)
    _check(lib.arah_sdf_grid(C.byref(frame.handle), C.c_int32(int(n_side)), _ptr(out), _ptr(buf), C.c_size_t(buf.numel()),
                             _stream()), "arah_sdf_grid")
    return out


_band_scratch = {}


@_guarded
def sdf_grid_band(frame, ws, n_side=256):
    """The lattice of sdf_grid for marching cubes at level 0: exact where the level set can pass, the right sign elsewhere
    (csrc/tier.hpp; ~6 % of the evaluations).  -> (volume (n_side,)*3, n_evaluated (1,) int32 on the device)."""
    lib = load_library()
    buf = ws.ensure(1, 1)
    dev = frame.device
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, int(n_side))
    sc = _band_scratch.get(key)
    if sc is None:
        if len(_band_scratch) >= 8:
            _band_scratch.pop(next(iter(_band_scratch)))
        sc = _band_scratch[key] = (torch.empty(int(lib.arah_sdf_grid_band_scratch_bytes()), dtype=torch.uint8, device=dev),
                                   torch.empty(n_side ** 3, dtype=torch.int32, device=dev))
    scratch, lst = sc
    out = torch.empty(n_side, n_side, n_side, device=dev)
    _check(lib.arah_sdf_grid_band(C.byref(frame.handle), C.c_int32(int(n_side)), _ptr(out), _ptr(lst), _ptr(scratch),
                                  C.c_size_t(scratch.numel()), _ptr(buf), C.c_size_t(buf.numel()), _stream()), "arah_sdf_grid_band")
    n_eval = scratch[0:4].view(torch.int32)
    return out, n_eval


POSED_FILL = 1.0   # ARAH_POSED_FILL (include/arah_hip.h), metres
POSED_WANT = ("sdf", "points_hat", "T", "normal", "weights")
_posed_scratch = {}


def _posed_buf(dev, nbytes):
    """Per-(device, stream) scratch of the posed queries (grows on demand; one stream's calls are ordered)."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    buf = _posed_scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is None and len(_posed_scratch) >= 8:
            _posed_scratch.pop(next(iter(_posed_scratch)))
        buf = _posed_scratch[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return buf


@_guarded
def query_posed(frame, ws, pts, occ=None, want=POSED_WANT):
    """The posed SDF at world points pts (P,3) (arah_query_posed): -> dict with `state` (P,) uint8 (0 not converged, 1 converged,
    2 skipped: certified sigma = +0 by the occupancy buffer `occ`) and the fields of `want` -- sdf (P,) metres, points_hat (P,3)
    normalised canonical, T (P,4,4), normal (P,3) posed unit normal, weights (P,24).  Skipped points have sdf = POSED_FILL and
    zeros in the other fields."""
    lib = load_library()
    x = _f32(pts).reshape(-1, 3)
    n, dev = int(x.shape[0]), frame.device
    bad = set(want) - set(POSED_WANT)
    if bad:
        raise ValueError("query_posed: unknown fields %s" % sorted(bad))
    sdf = torch.empty(n, device=dev)
    state = torch.empty(n, dtype=torch.uint8, device=dev)
    z = {"points_hat": 3, "T": 16, "normal": 3, "weights": 24}
    outs = {k: (torch.zeros(n, c, device=dev) if k in want else None) for k, c in z.items()}
    buf = _posed_buf(dev, lib.arah_query_posed_bytes(max(n, 1)))
    _check(lib.arah_query_posed(C.byref(frame.handle), _ptr(occ), _ptr(x), C.c_int32(n), _ptr(sdf), _ptr(outs["points_hat"]),
                                _ptr(outs["T"]), _ptr(outs["normal"]), _ptr(outs["weights"]), _ptr(state), _ptr(buf),
                                C.c_size_t(buf.numel()), _stream()), "arah_query_posed")
    res = {"state": state}
    if "sdf" in want:
        res["sdf"] = sdf
    for k in z:
        if k in want:
            res[k] = outs[k].reshape(n, 4, 4) if k == "T" else outs[k]
    return res


@_guarded
def sdf_grid_posed(frame, ws, n_side=256, occ=None, box=None, band=True):
    """The posed SDF (metres) on the n_side^3 lattice of a world cube (arah_sdf_grid_posed): converged points take their sdf,
    unconverged and skipped ones POSED_FILL.  box: (4,) device tensor (origin xyz, side) or None = the cube around the marked voxels
    of `occ`.  band: evaluate only the points that share a lattice cell with a marked one.  -> (volume (n,n,n) [ix,iy,iz],
    box (4,), counts (3,) int32 evaluated / converged / skipped), all on the device, no host round trip."""
    lib = load_library()
    dev, n_side = frame.device, int(n_side)
    if box is None and occ is None:
        raise ValueError("sdf_grid_posed: the default box needs the occupancy bitmap")
    if band and occ is None:
        raise ValueError("sdf_grid_posed: band=True needs the occupancy bitmap")
    out = torch.empty(n_side, n_side, n_side, device=dev)
    box_out = torch.empty(4, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    bx = _f32(box).reshape(4) if box is not None else None
    buf = _posed_buf(dev, lib.arah_sdf_grid_posed_bytes(n_side))
    _check(lib.arah_sdf_grid_posed(C.byref(frame.handle), _ptr(occ), _ptr(bx), C.c_int32(n_side), C.c_int32(1 if band else 0), _ptr(out),
                                   _ptr(box_out), _ptr(counts), _ptr(buf), C.c_size_t(buf.numel()), _stream()), "arah_sdf_grid_posed")
    return out, box_out, counts


def lattice_box(lo, hi, margin=0.0):
    """The cube (origin xyz, side) around the axis-aligned box [lo, hi] grown by `margin` on every side, centred on it (host
    helper of posed_mesh's `bounds`; the same rule k_posed_box_finish applies on the device)."""
    lo = torch.as_tensor(lo, dtype=torch.float32).reshape(3) - margin
    hi = torch.as_tensor(hi, dtype=torch.float32).reshape(3) + margin
    side = torch.max(hi - lo)
    return torch.cat([0.5 * (lo + hi) - 0.5 * side, side.reshape(1)])


def posed_band(marked):
    """Torch restatement of the lattice band of arah_sdf_grid_posed: marked (n,n,n) bool, lattice points in a marked voxel ->
    the points that share a lattice cell with one of them (their 3x3x3 neighbourhood), the points the band evaluates."""
    m = marked.float().reshape(1, 1, *marked.shape)
    return torch.nn.functional.max_pool3d(m, 3, stride=1, padding=1)[0, 0] > 0


def posed_value_rule(sdf, state):
    """The lattice's value rule: converged points (state 1) keep their sdf, unconverged (0) and skipped (2) ones take POSED_FILL."""
    return torch.where(state == 1, sdf, torch.full_like(sdf, POSED_FILL))


def lattice_to_world(x, box):
    """Coordinates in [-1,1]^3 of a lattice's marching cubes (arah_marching_cubes) -> world metres of the lattice `box`:
    point i / (n - 1) of the cube's side sits at -1 + 2 i / (n - 1) in the mesh."""
    return box[:3] + (x + 1.0) * (0.5 * box[3])


_mc_tables = {}


def _mc_device_tables(dev):
    """meshing.case_table() on `dev`, copied once: (tri_table (256,16) int8, n_tri (256,) int32)."""
    if dev not in _mc_tables:
        import numpy as np
        from . import meshing
        table_np, ntri_np = meshing.case_table()
        assert table_np.shape[1] <= 16
        t16 = -np.ones((256, 16), np.int8)
        t16[:, :table_np.shape[1]] = table_np
        _mc_tables[dev] = (torch.from_numpy(t16).to(dev), torch.from_numpy(ntri_np.astype(np.int32)).to(dev))
    return _mc_tables[dev]


MC_INDEXED_MAX_SIDE = 894   # the largest lattice whose edge keys (3 n^3 of them) fit int32
_mc_indexed_scratch = {}


def marching_cubes_indexed(sdf, level=0.0, vert_cap=1 << 19, face_cap=1 << 20, want_edge=False):
    """Level set of the lattice volume sdf (N,N,N) [ix,iy,iz] as an INDEXED mesh, on the device and WITHOUT a host round trip
    (arah_marching_cubes_indexed): one vertex per crossing lattice edge, in ascending order of the edge key
    ((ix N + iy) N + iz) 3 + axis.  -> verts (vert_cap,3) coordinates in [-1,1]^3, faces (face_cap,3) int32 vertex ids, counts
    (2,) int32 on the device (vertices and faces of the level set; either may exceed its capacity, then only the first rows
    were written), and with want_edge=True vert_edge (vert_cap,) int32, the vertices' keys.  Rows beyond the counts are zero.
    verts[faces] is `marching_cubes` of the same volume bit for bit; the result is meshing.marching_cubes_indexed(sdf).
    The scratch (4 N^3 bytes and the row tables) is kept per (device, stream) and grows on demand."""
    require_gpu()
    lib = load_library()
    v = _f32(sdf)
    if v.dim() != 3 or v.shape[0] != v.shape[1] or v.shape[0] != v.shape[2] or not 2 <= v.shape[0] <= MC_INDEXED_MAX_SIDE:
        raise ValueError("sdf must be an (N, N, N) lattice volume with 2 <= N <= %d" % MC_INDEXED_MAX_SIDE)
    if int(vert_cap) < 1 or int(face_cap) < 1:
        raise ValueError("vert_cap and face_cap must be at least 1")
    dev, N = v.device, int(v.shape[0])
    table, ntri = _mc_device_tables(dev)
    with _on_device(dev):
        need = int(lib.arah_marching_cubes_indexed_scratch_bytes(N))
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        scratch = _mc_indexed_scratch.get(key)
        if scratch is None or scratch.numel() < need:
            if scratch is None and len(_mc_indexed_scratch) >= 8:
                _mc_indexed_scratch.pop(next(iter(_mc_indexed_scratch)))
            scratch = _mc_indexed_scratch[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        verts = torch.empty(int(vert_cap), 3, device=dev)
        faces = torch.empty(int(face_cap), 3, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        vert_edge = torch.empty(int(vert_cap), dtype=torch.int32, device=dev) if want_edge else None
        _check(lib.arah_marching_cubes_indexed(_ptr(v), C.c_int32(N), C.c_float(float(level)), _ptr(table), _ptr(ntri), _ptr(verts),
                                               C.c_int32(int(vert_cap)), _ptr(vert_edge), _ptr(faces), C.c_int32(int(face_cap)),
                                               _ptr(counts), _ptr(scratch), C.c_size_t(scratch.numel()), _stream()),
               "arah_marching_cubes_indexed")
    return (verts, faces, counts, vert_edge) if want_edge else (verts, faces, counts)


_mesh_cc_scratch = {}


def _mesh_cc_buf(dev, nbytes):
    """Per-(device, stream) scratch of mesh_components / mesh_select (grows on demand; one stream's calls are ordered)."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    buf = _mesh_cc_scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is None and len(_mesh_cc_scratch) >= 8:
            _mesh_cc_scratch.pop(next(iter(_mesh_cc_scratch)))
        buf = _mesh_cc_scratch[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return buf


def _mesh_cc_args(faces, n_verts, what):
    """faces (F,3) integer ids on the GPU and the vertex count of a mesh_components / mesh_select call, checked: -> (faces int32
    contiguous, V, F)."""
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("%s: faces must be an (F, 3) tensor" % what)
    if faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == torch.bool:
        raise ValueError("%s: faces must hold integer vertex ids" % what)
    if not faces.is_cuda:
        raise ValueError("%s runs on the HIP kernels: faces must live on the GPU (meshing.%s is the host's)" % (what, what))
    if isinstance(n_verts, bool) or int(n_verts) != n_verts or not 0 <= int(n_verts) <= 2 ** 31 - 1:
        raise ValueError("%s: n_verts must be an integer in [0, 2^31), got %r" % (what, n_verts))
    if faces.dtype != torch.int32:
        # through int64, which holds every narrower type; ids that do not fit int32 are invalid anyway: they become -1, which the
        # kernels skip
        faces = faces.to(torch.int64)
        faces = torch.where((faces >= 0) & (faces <= 2 ** 31 - 1), faces, torch.full_like(faces, -1)).to(torch.int32)
    return faces.detach().contiguous(), int(n_verts), int(faces.shape[0])


def mesh_components(faces, n_verts):
    """Connected components of the indexed mesh with faces (F,3) integer vertex ids (on the GPU) over n_verts vertices
    (arah_mesh_components, csrc/meshcc.hpp): two vertices are connected when a face names both; a face with an id outside [0, n_verts)
    is skipped; a vertex no valid face names is a component of its own.  -> labels (V,) int32 dense component ids in [0, C),
    numbered in ascending order of the components' smallest vertex ids; comp_verts, comp_faces (V,) int32 sizes of component c, zero
    for c >= C; counts (3,) int32 = C, the valid faces, the component with the most faces (ties: the lowest id; -1 when C = 0).
    All on the device, no host synchronisation.  The result is meshing.mesh_components(faces, n_verts) bit for bit.  The scratch is
    kept per (device, stream) and grows on demand."""
    require_gpu()
    lib = load_library()
    f, V, F = _mesh_cc_args(faces, n_verts, "mesh_components")
    dev = f.device
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_components_scratch_bytes(V, F)))
        labels, comp_verts, comp_faces = (torch.empty(V, dtype=torch.int32, device=dev) for _ in range(3))
        counts = torch.empty(3, dtype=torch.int32, device=dev)
        _check(lib.arah_mesh_components(_ptr(f), C.c_int64(F), C.c_int64(V), _ptr(labels), _ptr(comp_verts), _ptr(comp_faces),
                                        _ptr(counts), _ptr(scratch), C.c_size_t(scratch.numel()), _stream()), "arah_mesh_components")
    return labels, comp_verts, comp_faces, counts


def mesh_select(faces, n_verts, labels, keep):
    """Order-preserving selection of the components with keep[c] != 0 (arah_mesh_select): labels (V,) from `mesh_components`, keep
    (V,) integer or bool indexed by component id.  -> vert_src (V,) int32 old id of new vertex j; vert_map (V,) int32 new id of old
    vertex v or -1; faces_out (F,3) int32 the kept valid faces in their order with the new ids; face_src (F,) int32 their old
    rows; counts (2,) int32 kept vertices, kept faces.  Rows beyond the counts are zero.  All on the device, no host
    synchronisation; the result is meshing.mesh_select(...) bit for bit."""
    require_gpu()
    lib = load_library()
    f, V, F = _mesh_cc_args(faces, n_verts, "mesh_select")
    dev = f.device
    for name, t in (("labels", labels), ("keep", keep)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (V,) or t.dtype.is_floating_point or t.dtype.is_complex:
            raise ValueError("mesh_select: %s must be an integer tensor of shape (%d,)" % (name, V))
        if t.device != dev:
            raise ValueError("mesh_select: %s lives on %s, faces on %s" % (name, t.device, dev))
    lab = labels.detach().to(torch.int32).contiguous()
    kp = (keep.detach() != 0).to(torch.int32).contiguous()
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_select_scratch_bytes(V, F)))
        vert_src, vert_map = (torch.empty(V, dtype=torch.int32, device=dev) for _ in range(2))
        faces_out = torch.empty(F, 3, dtype=torch.int32, device=dev)
        face_src = torch.empty(F, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        _check(lib.arah_mesh_select(_ptr(f), C.c_int64(F), C.c_int64(V), _ptr(lab), _ptr(kp), _ptr(vert_src), _ptr(vert_map),
                                    _ptr(faces_out), _ptr(face_src), _ptr(counts), _ptr(scratch), C.c_size_t(scratch.numel()),
                                    _stream()), "arah_mesh_select")
    return vert_src, vert_map, faces_out, face_src, counts


def mesh_simplify(verts, faces, origin, cell, dims, position="mean", dedup=True):
    """Vertex clustering of an indexed mesh on a grid (arah_mesh_simplify, csrc/meshsimp.hpp): verts (V,3) float32 and faces (F,3)
    integer ids on the GPU; origin (three numbers), cell and dims (three integers, at most 2^27 cells) on the host.  The vertices of
    every occupied cell become one vertex, at the exact mean of the cell's members (position="mean") or at the member nearest to it
    (position="member"); faces that name an invalid vertex, collapse or (dedup) repeat an earlier face's three clusters go.  ->
    verts_out (V,3) float32, vert_src (V,) int32 the representative member of every cluster, vert_map (V,) int32 the cluster of
    every vertex or -1, faces_out (F,3) int32, face_src (F,) int32, counts (6,) int32 = clusters, kept faces, invalid, collapsed,
    duplicate faces, status (1: dedup with more than 2^21 clusters, no face kept).  Rows beyond the counts are zero.  All on the
    device, no host synchronisation; the result is meshing.mesh_simplify(...) bit for bit."""
    from . import meshing
    require_gpu()
    lib = load_library()
    if position not in ("mean", "member"):
        raise ValueError("mesh_simplify: position must be 'mean' or 'member', got %r" % (position,))
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("mesh_simplify: verts must be a (V, 3) float32 tensor")
    V = int(verts.shape[0])
    f, _, F = _mesh_cc_args(faces, V, "mesh_simplify")
    if verts.device != f.device:
        raise ValueError("mesh_simplify: verts live on %s, faces on %s" % (verts.device, f.device))
    if V > meshing.SIMPLIFY_MAX_VERTS or F > meshing.SIMPLIFY_MAX_FACES:
        raise ValueError("mesh_simplify: at most 2^26 vertices and 2^28 faces, got %d and %d" % (V, F))
    o, c, _, d, scale = meshing.simplify_grid(origin, cell, dims)
    dev = f.device
    v = verts.detach().contiguous()
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_simplify_scratch_bytes(V, F, d[0] * d[1] * d[2])))
        verts_out = torch.empty(V, 3, dtype=torch.float32, device=dev)
        vert_src, vert_map = (torch.empty(V, dtype=torch.int32, device=dev) for _ in range(2))
        faces_out = torch.empty(F, 3, dtype=torch.int32, device=dev)
        face_src = torch.empty(F, dtype=torch.int32, device=dev)
        counts = torch.empty(6, dtype=torch.int32, device=dev)
        _check(lib.arah_mesh_simplify(_ptr(v), C.c_int64(V), _ptr(f), C.c_int64(F), (C.c_float * 3)(*o), C.c_float(c),
                                      (C.c_int32 * 3)(*d), C.c_double(scale), C.c_int32(int(position == "member")),
                                      C.c_int32(int(bool(dedup))), _ptr(verts_out), _ptr(vert_src), _ptr(vert_map), _ptr(faces_out),
                                      _ptr(face_src), _ptr(counts), _ptr(scratch), C.c_size_t(scratch.numel()), _stream()),
               "arah_mesh_simplify")
    return verts_out, vert_src, vert_map, faces_out, face_src, counts


def mesh_quadric_place(verts, faces, vert_map, means, n_clusters, cell, reg=1e-3):
    """Quadric-error placement of the clusters of `mesh_simplify` (arah_mesh_quadric_place, csrc/meshquadric.hpp): verts (V,3)
    float32, faces (F,3) integer ids, vert_map (V,) and means (V,3) float32 (verts_out at position="mean") of mesh_simplify on the
    GPU; n_clusters its counts (K is read at [0] ON THE DEVICE) or an integer; cell the cell length, reg >= 0 the share of the
    quadric's trace that pulls a cluster towards its mean.  -> pos (V,3) float32, vert_src (V,) int32 the member nearest to pos,
    qcounts (4,) int32 = clusters that fell back to the mean, (face, cluster) pairs, the longest segment, status (2: a cluster
    with more than 2^15 pairs was not placed).  Rows from K on are zero.  All on the device, no host synchronisation; the result
    is meshing.mesh_quadric_place(...) bit for bit."""
    from . import meshing
    require_gpu()
    lib = load_library()
    what = "mesh_quadric_place"
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("%s: verts must be a (V, 3) float32 tensor" % what)
    V = int(verts.shape[0])
    f, _, F = _mesh_cc_args(faces, V, what)
    if V > meshing.SIMPLIFY_MAX_VERTS or F > meshing.SIMPLIFY_MAX_FACES:
        raise ValueError("%s: at most 2^26 vertices and 2^28 faces, got %d and %d" % (what, V, F))
    if not isinstance(means, torch.Tensor) or tuple(means.shape) != (V, 3) or means.dtype != torch.float32:
        raise ValueError("%s: means must be a (%d, 3) float32 tensor" % (what, V))
    if (not isinstance(vert_map, torch.Tensor) or tuple(vert_map.shape) != (V,) or vert_map.dtype.is_floating_point
            or vert_map.dtype.is_complex or vert_map.dtype == torch.bool):
        raise ValueError("%s: vert_map must be an integer tensor of shape (%d,)" % (what, V))
    dev = f.device
    if verts.device != dev or means.device != dev or vert_map.device != dev:
        raise ValueError("%s: verts, faces, vert_map and means must live on one device" % what)
    on_device = isinstance(n_clusters, torch.Tensor) and n_clusters.device == dev
    K, c, reg = meshing.quadric_args(0 if on_device else n_clusters, cell, reg, V, what)
    if on_device:                    # the counts of mesh_simplify stay where they are: K is read by the kernels
        if n_clusters.dtype.is_floating_point or n_clusters.numel() < 1:
            raise ValueError("%s: n_clusters must be an integer or the counts of mesh_simplify" % what)
        counts = n_clusters.detach().reshape(-1)[:1].to(torch.int32).contiguous()
    else:
        counts = torch.tensor([K], dtype=torch.int32, device=dev)
    vm = vert_map.detach()
    if vm.dtype != torch.int32:      # a cluster id that does not fit int32 is no cluster: -1
        vm = vm.to(torch.int64)
        vm = torch.where((vm >= 0) & (vm <= 2 ** 31 - 1), vm, torch.full_like(vm, -1)).to(torch.int32)
    v, mn, vm = verts.detach().contiguous(), means.detach().contiguous(), vm.contiguous()
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_quadric_place_scratch_bytes(V, F)))
        pos = torch.empty(V, 3, dtype=torch.float32, device=dev)
        vert_src = torch.empty(V, dtype=torch.int32, device=dev)
        qcounts = torch.empty(4, dtype=torch.int32, device=dev)
        _check(lib.arah_mesh_quadric_place(_ptr(v), C.c_int64(V), _ptr(f), C.c_int64(F), _ptr(vm), _ptr(mn), _ptr(counts), C.c_float(c),
                                           C.c_double(reg), _ptr(pos), _ptr(vert_src), _ptr(qcounts), _ptr(scratch),
                                           C.c_size_t(scratch.numel()), _stream()), "arah_mesh_quadric_place")
    return pos, vert_src, qcounts


def mesh_adjacency(faces, n_verts):
    """Adjacency of the indexed mesh with faces (F,3) integer vertex ids (on the GPU) over n_verts vertices (arah_mesh_adjacency,
    csrc/meshadj.hpp): -> (vf_start (V+1,), vf (3F,), nbr_start (V+1,), nbr (6F,), nbr_out (6F,), nbr_in (6F,)) int32, vert_flags (V,)
    uint8, counts (8,) int32 as meshing.mesh_adjacency describes them, and equal to it bit for bit.  All on the device, no host
    synchronisation.  The scratch is kept per (device, stream) and grows on demand."""
    from . import meshing
    require_gpu()
    lib = load_library()
    f, V, F = _mesh_cc_args(faces, n_verts, "mesh_adjacency")
    if F > meshing.ADJACENCY_MAX_FACES:
        raise ValueError("mesh_adjacency: at most 2^28 faces, got %d" % F)
    dev, i32 = f.device, torch.int32
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_adjacency_scratch_bytes(V, F)))
        vf_start, nbr_start = (torch.empty(V + 1, dtype=i32, device=dev) for _ in range(2))
        vf = torch.empty(3 * F, dtype=i32, device=dev)
        nbr, nbr_out, nbr_in = (torch.empty(6 * F, dtype=i32, device=dev) for _ in range(3))
        flags = torch.empty(V, dtype=torch.uint8, device=dev)
        counts = torch.empty(8, dtype=i32, device=dev)
        _check(lib.arah_mesh_adjacency(_ptr(f), C.c_int64(F), C.c_int64(V), _ptr(vf_start), _ptr(vf), _ptr(nbr_start), _ptr(nbr),
                                       _ptr(nbr_out), _ptr(nbr_in), _ptr(flags), _ptr(counts), _ptr(scratch),
                                       C.c_size_t(scratch.numel()), _stream()), "arah_mesh_adjacency")
    return vf_start, vf, nbr_start, nbr, nbr_out, nbr_in, flags, counts


def _mesh_verts_faces(verts, faces, what, bounded=True):
    """verts (V,3) float32 and faces (F,3) integer ids on one GPU, at most meshing.ADJACENCY_MAX_FACES faces (bounded=False: the
    caller has a bound of its own): -> (verts contiguous, faces int32 contiguous, V, F)."""
    from . import meshing
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("%s: verts must be a (V, 3) float32 tensor" % what)
    V = int(verts.shape[0])
    f, _, F = _mesh_cc_args(faces, V, what)
    if verts.device != f.device:
        raise ValueError("%s: verts live on %s, faces on %s" % (what, verts.device, f.device))
    if bounded and F > meshing.ADJACENCY_MAX_FACES:
        raise ValueError("%s: at most 2^28 faces, got %d" % (what, F))
    return verts.detach().contiguous(), f, V, F


def _mesh_adj_args(verts, faces, adjacency, what):
    """verts (V,3) float32 and faces on one GPU, and the eight arrays of mesh_adjacency (built here when None): -> (verts
    contiguous, faces int32 contiguous, V, F, adjacency as contiguous device arrays)."""
    v, f, V, F = _mesh_verts_faces(verts, faces, what)
    return v, f, V, F, _mesh_adj_arrays(f, V, F, adjacency, what)


def _mesh_adj_only(faces, n_verts, adjacency, what):
    """faces on the GPU over n_verts vertices and the eight arrays of mesh_adjacency (built here when None): -> (faces int32
    contiguous, V, F, adjacency as contiguous device arrays)."""
    from . import meshing
    f, V, F = _mesh_cc_args(faces, n_verts, what)
    if F > meshing.ADJACENCY_MAX_FACES:
        raise ValueError("%s: at most 2^28 faces, got %d" % (what, F))
    return f, V, F, _mesh_adj_arrays(f, V, F, adjacency, what)


def _mesh_adj_arrays(f, V, F, adjacency, what):
    """The eight arrays of mesh_adjacency of the checked faces f (built here when None), checked: -> contiguous device arrays."""
    if adjacency is None:
        return mesh_adjacency(f, V)
    adjacency = tuple(adjacency)
    shapes = ((V + 1,), (3 * F,), (V + 1,), (6 * F,), (6 * F,), (6 * F,), (V,), (8,))
    if len(adjacency) != 8 or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != s or t.device != f.device
                                  or t.dtype != (torch.uint8 if i == 6 else torch.int32)
                                  for i, (t, s) in enumerate(zip(adjacency, shapes))):
        raise ValueError("%s: adjacency must be the eight arrays of mesh_adjacency of these faces and vertices, on %s" % (what, f.device))
    return tuple(t.contiguous() for t in adjacency)


def mesh_collapse_round(verts, faces, need, reg=1e-3, max_cost=float("inf"), details=False, short_len2=None, long_len2=None):
    """One round of edge-collapse decimation (arah_mesh_collapse_round, csrc/meshcollapse.hpp): verts (V,3) float32 and faces (F,3)
    integer ids on the GPU; need, reg and max_cost on the host, as meshing.mesh_collapse_round describes them.  The adjacency of
    the mesh is built inside the call.  -> verts_out (V,3) float32, faces_out (F,3) int32, vert_src (V,) int32, face_src (F,) int32,
    counts (12,) int32 (meshing.COLLAPSE_COUNTS); rows past the counts are zero; details: also edge_pos (6F,3) float32, edge_key
    (6F,) int64 and edge_reason (6F,) uint8 of every neighbour entry.  short_len2 / long_len2: the two length bounds
    (arah_mesh_collapse_round_bounded, the same kernels; counts (14,), meshing.COLLAPSE_BOUNDED_COUNTS).  All on the device, no host
    synchronisation; the result is meshing.mesh_collapse_round(...) bit for bit."""
    from . import meshing
    require_gpu()
    lib = load_library()
    what = "mesh_collapse_round"
    need, reg, max_cost = meshing.collapse_args(need, reg, max_cost, what)
    bounds = meshing.collapse_bounds(short_len2, long_len2, what)
    v, f, V, F = _mesh_verts_faces(verts, faces, what)
    dev, i32 = f.device, torch.int32
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_collapse_round_scratch_bytes(V, F)))
        verts_out = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces_out = torch.empty(F, 3, dtype=i32, device=dev)
        vert_src, face_src = torch.empty(V, dtype=i32, device=dev), torch.empty(F, dtype=i32, device=dev)
        counts = torch.empty(len(meshing.COLLAPSE_COUNTS if bounds is None else meshing.COLLAPSE_BOUNDED_COUNTS), dtype=i32, device=dev)
        edge_pos = torch.empty(6 * F, 3, dtype=torch.float32, device=dev)
        edge_key = torch.empty(6 * F, dtype=torch.int64, device=dev)
        edge_reason = torch.empty(6 * F, dtype=torch.uint8, device=dev)
        # the two entries differ by the two bounds, which the bounded one takes after max_cost
        name = "arah_mesh_collapse_round" if bounds is None else "arah_mesh_collapse_round_bounded"
        lens = () if bounds is None else (C.c_double(bounds[0]), C.c_double(bounds[1]))
        _check(getattr(lib, name)(_ptr(v), C.c_int64(V), _ptr(f), C.c_int64(F), C.c_int32(need), C.c_double(reg), C.c_float(max_cost),
                                  *lens, _ptr(verts_out), _ptr(faces_out), _ptr(vert_src), _ptr(face_src), _ptr(counts),
                                  _ptr(edge_pos), _ptr(edge_key), _ptr(edge_reason), _ptr(scratch), C.c_size_t(scratch.numel()),
                                  _stream()), name)
    out = (verts_out, faces_out, vert_src, face_src, counts)
    return out + (edge_pos, edge_key, edge_reason) if details else out


def mesh_subdivide_round(verts, faces, method="midpoint", max_len2=None):
    """One round of subdivision (arah_mesh_subdivide_round, csrc/meshsubdiv.hpp): verts (V,3) float32 and faces (F,3) integer ids on
    the GPU; method "midpoint" or "loop" and max_len2 (None: every edge; a float: the edges with a squared length above it,
    midpoint only) on the host, as meshing.mesh_subdivide_round describes them.  The adjacency of the mesh is built inside the
    call.  -> verts_out (V+3F,3) float32, faces_out (4F,3) int32, vert_src (V+3F,2) int32, face_src (4F,) int32, counts (13,)
    int32 (meshing.SUBDIVIDE_COUNTS); rows past the counts are zero.  All on the device, no host synchronisation; the result is
    meshing.mesh_subdivide_round(...) bit for bit."""
    from . import meshing
    require_gpu()
    lib = load_library()
    what = "mesh_subdivide_round"
    v, f, V, F = _mesh_verts_faces(verts, faces, what, bounded=False)   # subdivide_args holds the bound on F, with V
    loop, max_len2 = meshing.subdivide_args(method, max_len2, V, F, what)
    dev, i32 = f.device, torch.int32
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_subdivide_round_scratch_bytes(V, F)))
        verts_out = torch.empty(V + 3 * F, 3, dtype=torch.float32, device=dev)
        faces_out = torch.empty(4 * F, 3, dtype=i32, device=dev)
        vert_src, face_src = torch.empty(V + 3 * F, 2, dtype=i32, device=dev), torch.empty(4 * F, dtype=i32, device=dev)
        counts = torch.empty(len(meshing.SUBDIVIDE_COUNTS), dtype=i32, device=dev)
        _check(lib.arah_mesh_subdivide_round(_ptr(v), C.c_int64(V), _ptr(f), C.c_int64(F), C.c_int32(loop),
                                             C.c_int32(0 if max_len2 is None else 1), C.c_double(0.0 if max_len2 is None else max_len2),
                                             _ptr(verts_out), _ptr(faces_out), _ptr(vert_src), _ptr(face_src), _ptr(counts),
                                             _ptr(scratch), C.c_size_t(scratch.numel()), _stream()), "arah_mesh_subdivide_round")
    return verts_out, faces_out, vert_src, face_src, counts


def mesh_flip_round(verts, faces, criterion="delaunay", salt=0, details=False):
    """One round of edge flips (arah_mesh_flip_round, csrc/meshflip.hpp): verts (V,3) float32 and faces (F,3) integer ids on the
    GPU; criterion "delaunay" or "valence" and salt (the round number) on the host, as meshing.mesh_flip_round describes them.  The
    adjacency of the mesh is built inside the call.  -> faces_out (F,3) int32, face_flag (F,) uint8, counts (9,) int32
    (meshing.FLIP_COUNTS); details: also edge_key (6F,) int64 and edge_reason (6F,) uint8 of every neighbour entry.  All on the
    device, no host synchronisation; the result is meshing.mesh_flip_round(...) bit for bit."""
    from . import meshing
    require_gpu()
    lib = load_library()
    what = "mesh_flip_round"
    crit, salt = meshing.flip_args(criterion, salt, what)
    v, f, V, F = _mesh_verts_faces(verts, faces, what)
    dev, i32 = f.device, torch.int32
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_flip_round_scratch_bytes(V, F)))
        faces_out = torch.empty(F, 3, dtype=i32, device=dev)
        face_flag = torch.empty(F, dtype=torch.uint8, device=dev)
        counts = torch.empty(len(meshing.FLIP_COUNTS), dtype=i32, device=dev)
        edge_key = torch.empty(6 * F, dtype=torch.int64, device=dev)
        edge_reason = torch.empty(6 * F, dtype=torch.uint8, device=dev)
        _check(lib.arah_mesh_flip_round(_ptr(v), C.c_int64(V), _ptr(f), C.c_int64(F), C.c_int32(crit), C.c_uint32(salt),
                                        _ptr(faces_out), _ptr(face_flag), _ptr(counts), _ptr(edge_key), _ptr(edge_reason),
                                        _ptr(scratch), C.c_size_t(scratch.numel()), _stream()), "arah_mesh_flip_round")
    out = (faces_out, face_flag, counts)
    return out + (edge_key, edge_reason) if details else out


def vertex_normals(verts, faces, adjacency=None):
    """Per-vertex normals of an indexed mesh from the mesh itself (arah_mesh_vertex_normals): verts (V,3) float32 and faces (F,3)
    integer ids on the GPU, adjacency: `mesh_adjacency` of them, or None to build it here.  -> normal_sum (V,3) float64 (the
    incident faces' cross products summed in ascending face id), normals (V,3) float32 (unit, or zero); meshing.vertex_normals bit
    for bit.  A gather over the sorted CSR: no atomics, no host synchronisation."""
    require_gpu()
    lib = load_library()
    v, f, V, F, adj = _mesh_adj_args(verts, faces, adjacency, "vertex_normals")
    dev = v.device
    with _on_device(dev):
        normal_sum = torch.empty(V, 3, dtype=torch.float64, device=dev)
        normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
        _check(lib.arah_mesh_vertex_normals(_ptr(v), C.c_int64(V), _ptr(f), C.c_int64(F), _ptr(adj[0]), _ptr(adj[1]),
                                            _ptr(normal_sum), _ptr(normals), _stream()), "arah_mesh_vertex_normals")
    return normal_sum, normals


def mesh_smooth(verts, faces, iterations, lamb=0.5, mu=-0.53, method="taubin", boundary="pin", adjacency=None, weights="uniform"):
    """Laplacian / Taubin umbrella smoothing of an indexed mesh (arah_mesh_smooth): verts (V,3) float32 and faces (F,3) integer ids
    on the GPU, the keywords of meshing.mesh_smooth, adjacency: `mesh_adjacency` of them, or None to build it here.  ->
    verts_out (V,3) float32, meshing.mesh_smooth bit for bit.  All steps inside one C call, between two buffers; no atomics, no
    host synchronisation.  weights="cotangent": arah_mesh_smooth_cotangent, the weights of every step in the call's scratch."""
    from . import meshing
    require_gpu()
    lib = load_library()
    factors, pin = meshing.check_smooth_args(iterations, lamb, mu, method, boundary)
    meshing.check_smooth_weights(weights)
    v, f, V, F, adj = _mesh_adj_args(verts, faces, adjacency, "mesh_smooth")
    dev = v.device
    n_steps = int(iterations) * len(factors)
    if n_steps > 2 ** 31 - 1:
        raise ValueError("mesh_smooth: too many steps, got %d iterations" % iterations)
    with _on_device(dev):
        out = torch.empty(V, 3, dtype=torch.float32, device=dev)
        tmp = torch.empty(V, 3, dtype=torch.float32, device=dev) if n_steps > 1 else None
        if weights == "cotangent":
            scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_smooth_cotangent_scratch_bytes(V, F)))
            _check(lib.arah_mesh_smooth_cotangent(_ptr(v), C.c_int64(V), _ptr(f), C.c_int64(F), _ptr(adj[0]), _ptr(adj[1]), _ptr(adj[2]),
                                                  _ptr(adj[3]), _ptr(adj[6]), C.c_int32(n_steps),
                                                  (C.c_float * 2)(factors[0], factors[-1]), C.c_int32(int(pin)), _ptr(tmp), _ptr(out),
                                                  _ptr(scratch), C.c_size_t(scratch.numel()), _stream()), "arah_mesh_smooth_cotangent")
            return out
        _check(lib.arah_mesh_smooth(_ptr(v), C.c_int64(V), _ptr(adj[2]), _ptr(adj[3]), _ptr(adj[6]), C.c_int32(n_steps),
                                    (C.c_float * 2)(factors[0], factors[-1]), C.c_int32(int(pin)), _ptr(tmp), _ptr(out), _stream()),
               "arah_mesh_smooth")
    return out


def mesh_tangential_step(verts, faces, normal_sum, lamb=0.5, adjacency=None):
    """One step of tangential relaxation (arah_mesh_tangential): verts (V,3) float32, faces (F,3) integer ids and normal_sum (V,3)
    float64 (vertex_normals' first output for the same mesh) on the GPU, lamb as meshing.mesh_tangential_step describes it,
    adjacency: `mesh_adjacency` of the mesh, or None to build it here.  -> verts_out (V,3) float32, meshing.mesh_tangential_step
    bit for bit.  A gather: no atomics, no host synchronisation."""
    from . import meshing
    require_gpu()
    lib = load_library()
    what = "mesh_tangential_step"
    factor = meshing.check_tangential_lamb(lamb, what)
    v, f, V, F, adj = _mesh_adj_args(verts, faces, adjacency, what)
    dev = v.device
    if not isinstance(normal_sum, torch.Tensor) or tuple(normal_sum.shape) != (V, 3) or normal_sum.dtype != torch.float64 \
            or normal_sum.device != dev:
        raise ValueError("%s: normal_sum must be the (V, 3) float64 sum of vertex_normals, on %s" % (what, dev))
    with _on_device(dev):
        out = torch.empty(V, 3, dtype=torch.float32, device=dev)
        _check(lib.arah_mesh_tangential(_ptr(v), C.c_int64(V), _ptr(adj[2]), _ptr(adj[3]), _ptr(adj[6]), _ptr(normal_sum.contiguous()),
                                        C.c_float(factor), _ptr(out), _stream()), "arah_mesh_tangential")
    return out


def mesh_cotangent(verts, faces, mass="mixed", adjacency=None):
    """The cotangent Laplacian of an indexed mesh (arah_mesh_cotangent, csrc/meshlaplace.hpp): verts (V,3) float32 and faces (F,3)
    integer ids on the GPU, mass "barycentric" or "mixed", adjacency: `mesh_adjacency` of them, or None to build it here.  ->
    weight (6F,), diag, area, angle_sum (V,) float64 and counts (8,) int32 as meshing.mesh_cotangent describes them: bit for bit,
    except angle_sum by the device's atan2.  A gather: no floating-point atomics, no host synchronisation."""
    from . import meshing
    require_gpu()
    lib = load_library()
    m = meshing.check_mass(mass)
    v, f, V, F, adj = _mesh_adj_args(verts, faces, adjacency, "mesh_cotangent")
    dev, f64 = v.device, torch.float64
    with _on_device(dev):
        weight = torch.empty(6 * F, dtype=f64, device=dev)
        diag, area, angle_sum = (torch.empty(V, dtype=f64, device=dev) for _ in range(3))
        counts = torch.empty(8, dtype=torch.int32, device=dev)
        _check(lib.arah_mesh_cotangent(_ptr(v), C.c_int64(V), _ptr(f), C.c_int64(F), _ptr(adj[0]), _ptr(adj[1]), _ptr(adj[2]),
                                       _ptr(adj[3]), C.c_int32(m), _ptr(weight), _ptr(diag), _ptr(area), _ptr(angle_sum), _ptr(counts),
                                       _stream()), "arah_mesh_cotangent")
    return weight, diag, area, angle_sum, counts


def _laplacian_args(weight, adjacency, what):
    adjacency = tuple(adjacency) if adjacency is not None else ()
    if len(adjacency) != 8 or any(not isinstance(t, torch.Tensor) or not t.is_cuda for t in adjacency):
        raise ValueError("%s: adjacency must be the eight arrays of mesh_adjacency, on the GPU" % what)
    nbr_start, nbr = adjacency[2], adjacency[3]
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float64 or weight.shape != nbr.shape or weight.device != nbr.device \
            or nbr_start.dtype != torch.int32 or nbr.dtype != torch.int32 or nbr_start.dim() != 1 or nbr_start.shape[0] < 1 \
            or nbr.dim() != 1 or nbr.shape[0] % 6 or nbr_start.device != nbr.device:
        raise ValueError("%s: weight must be the (6F,) float64 weights of mesh_cotangent, beside nbr" % what)
    return weight.detach().contiguous(), nbr_start.contiguous(), nbr.contiguous(), int(nbr_start.shape[0]) - 1, int(nbr.shape[0]) // 6


def laplacian_apply(weight, adjacency, x):
    """y = L x (arah_mesh_laplacian_apply): weight of `mesh_cotangent`, adjacency `mesh_adjacency`, x (V,C) float32 or float64 with
    1 <= C <= 32, all on one GPU.  -> y (V,C) float64, meshing.laplacian_apply bit for bit."""
    from . import meshing
    require_gpu()
    lib = load_library()
    w, nbr_start, nbr, V, F = _laplacian_args(weight, adjacency, "laplacian_apply")
    x = meshing._laplacian_x(x, V, w.device, "laplacian_apply").contiguous()
    dev = w.device
    with _on_device(dev):
        y = torch.empty(V, x.shape[1], dtype=torch.float64, device=dev)
        _check(lib.arah_mesh_laplacian_apply(_ptr(w), _ptr(nbr_start), _ptr(nbr), C.c_int64(V), C.c_int64(F), _ptr(x),
                                             C.c_int32(int(x.dtype == torch.float64)), C.c_int32(int(x.shape[1])), _ptr(y), _stream()),
               "arah_mesh_laplacian_apply")
    return y


def mesh_curvature(verts, faces, mass="mixed", adjacency=None, laplacian=None, normal_sum=None):
    """Mean, Gaussian and principal curvatures at the vertices (arah_mesh_curvature): verts (V,3) float32 and faces (F,3) integer ids
    on the GPU, and what meshing.mesh_curvature takes; whatever is None is computed here.  -> curv (V,5) float64 (mean, mean_abs,
    gaussian, k1, k2), mean_normal (V,3) float64, valid (V,) uint8, counts (1,) int32: meshing.mesh_curvature bit for bit given
    the same angle_sum.  Square roots and divisions happen on the device."""
    from . import meshing
    require_gpu()
    lib = load_library()
    what = "mesh_curvature"
    meshing.check_mass(mass, what)
    v, f, V, F, adj = _mesh_adj_args(verts, faces, adjacency, what)
    dev, f64 = v.device, torch.float64
    if laplacian is None:
        laplacian = mesh_cotangent(v, f, mass, adj)
    weight, _, area, angle_sum = tuple(laplacian)[:4]
    if normal_sum is None:
        normal_sum = vertex_normals(v, f, adj)[0]
    for t, shape in ((weight, (6 * F,)), (area, (V,)), (angle_sum, (V,)), (normal_sum, (V, 3))):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != f64 or t.device != dev:
            raise ValueError("%s: laplacian must be the outputs of mesh_cotangent, normal_sum of vertex_normals, on %s" % (what, dev))
    with _on_device(dev):
        curv = torch.empty(V, 5, dtype=f64, device=dev)
        mean_normal = torch.empty(V, 3, dtype=f64, device=dev)
        valid = torch.empty(V, dtype=torch.uint8, device=dev)
        counts = torch.empty(1, dtype=torch.int32, device=dev)
        _check(lib.arah_mesh_curvature(_ptr(v), C.c_int64(V), C.c_int64(F), _ptr(adj[2]), _ptr(adj[3]), _ptr(adj[6]),
                                       _ptr(weight.contiguous()), _ptr(area.contiguous()), _ptr(angle_sum.contiguous()),
                                       _ptr(normal_sum.contiguous()), _ptr(curv), _ptr(mean_normal), _ptr(valid), _ptr(counts),
                                       _stream()), "arah_mesh_curvature")
    return curv, mean_normal, valid, counts


def laplacian_solve(weight, area, adjacency, rhs, x0, pinned=None, mass_coef=0.0, stiff_coef=1.0, tol=1e-10, max_iter=10000,
                    check_every=32):
    """Jacobi-preconditioned conjugate gradients with the cotangent operator (arah_mesh_solve_begin / arah_mesh_solve_steps,
    csrc/meshsolve.hpp): the arguments of meshing.laplacian_solve, everything on one GPU.  -> x (V,C) float64, iters, status (C,)
    int32, rr, r0 (C,) float64, counts (8,) int32, classes (V,) uint8: meshing.laplacian_solve bit for bit.  The steps are
    launched in batches of check_every, four launches a step, and the C statuses are read once per batch -- the only host
    synchronisations; the iterate never goes to the host.  A column that stops inside a batch is left alone by the steps after it,
    so the batching does not show in the result."""
    from . import meshing
    require_gpu()
    lib = load_library()
    what = "laplacian_solve"
    mc, sc, tol, max_iter = meshing.check_solve_args(mass_coef, stiff_coef, tol, max_iter, what)
    if isinstance(check_every, bool) or not isinstance(check_every, int) or check_every < 1:
        raise ValueError("%s: check_every must be an integer >= 1, got %r" % (what, check_every))
    w, nbr_start, nbr, V, F = _laplacian_args(weight, adjacency, what)
    dev = w.device
    n_ch = meshing.check_solve_tensors(area, rhs, x0, pinned, V, dev, what)
    area, rhs, x0 = area.detach().contiguous(), rhs.detach().contiguous(), x0.detach().contiguous()
    pin = pinned.to(torch.uint8).contiguous() if pinned is not None else None
    with _on_device(dev):
        x = torch.empty(V, n_ch, dtype=torch.float64, device=dev)
        iters, status = (torch.empty(n_ch, dtype=torch.int32, device=dev) for _ in range(2))
        rr, r0 = (torch.empty(n_ch, dtype=torch.float64, device=dev) for _ in range(2))
        counts = torch.empty(8, dtype=torch.int32, device=dev)
        classes = torch.empty(V, dtype=torch.uint8, device=dev)
        nbytes = int(lib.arah_mesh_solve_scratch_bytes(V, n_ch))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)              # the state of this solve: its own, not the shared buffer
        op = (_ptr(w), _ptr(area), _ptr(nbr_start), _ptr(nbr), C.c_int64(V), C.c_int64(F))
        coef = (C.c_double(mc), C.c_double(sc))
        _check(lib.arah_mesh_solve_begin(*op, _ptr(rhs), _ptr(x0), _ptr(pin), C.c_int32(n_ch), *coef, C.c_double(tol), _ptr(x),
                                         _ptr(iters), _ptr(status), _ptr(rr), _ptr(r0), _ptr(counts), _ptr(classes), _ptr(scratch),
                                         C.c_size_t(nbytes), _stream()), "arah_mesh_solve_begin")
        done = 0
        while done < max_iter and bool((status == 0).any()):                      # one synchronisation per batch
            n = min(int(check_every), max_iter - done)
            _check(lib.arah_mesh_solve_steps(*op, C.c_int32(n_ch), *coef, C.c_int32(n), _ptr(x), _ptr(iters), _ptr(status), _ptr(rr),
                                             _ptr(r0), _ptr(scratch), C.c_size_t(nbytes), _stream()), "arah_mesh_solve_steps")
            done += n
    return x, iters, status, rr, r0, counts, classes


def mesh_orient(verts, faces, policy="majority", adjacency=None, quant=None):
    """Consistent orientation of an indexed mesh (arah_mesh_orient, csrc/meshorient.hpp): verts (V,3) float32 on the GPU -- or the
    vertex count under "seed" and "majority" --, faces (F,3) integer ids on the GPU, adjacency: `mesh_adjacency` of them, or None to
    build it here.  -> flip (F,) uint8, face_comp (F,) int32, faces_out (F,3) int32, comp_faces, comp_flags (F,) int32,
    comp_vol_hi, comp_vol_lo (F,) int64, counts (6,) int32 as meshing.mesh_orient describes them, and equal to it bit for bit.  No
    host synchronisation under "seed" and "majority"; the two volume policies read the vertices' bounds once
    (meshing.orient_quant) unless `quant` is given."""
    from . import meshing
    require_gpu()
    lib = load_library()
    pol = meshing.check_orient_policy(policy)
    if isinstance(verts, torch.Tensor) and verts.dim() > 0:
        if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
            raise ValueError("mesh_orient: verts must be a (V, 3) float32 tensor")
        v, n_verts = verts.detach().contiguous(), int(verts.shape[0])
    else:
        v, n_verts = None, verts
    if pol >= 2 and v is None:
        raise ValueError("mesh_orient: policy %r needs the vertices, not their number" % (policy,))
    f, V, F, adj = _mesh_adj_only(faces, n_verts, adjacency, "mesh_orient")
    if v is not None and v.device != f.device:
        raise ValueError("mesh_orient: verts live on %s, faces on %s" % (v.device, f.device))
    origin, scale = ([0.0, 0.0, 0.0], 1.0)
    if pol >= 2:
        origin, scale = meshing._check_quant(meshing.orient_quant(v) if quant is None else quant, "mesh_orient")
    dev, i32, i64 = f.device, torch.int32, torch.int64
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_orient_scratch_bytes(V, F)))
        flip = torch.empty(F, dtype=torch.uint8, device=dev)
        face_comp, comp_faces, comp_flags = (torch.empty(F, dtype=i32, device=dev) for _ in range(3))
        faces_out = torch.empty(F, 3, dtype=i32, device=dev)
        vol_hi, vol_lo = (torch.empty(F, dtype=i64, device=dev) for _ in range(2))
        counts = torch.empty(6, dtype=i32, device=dev)
        _check(lib.arah_mesh_orient(_ptr(v) if pol >= 2 else None, C.c_int64(V), _ptr(f), C.c_int64(F), _ptr(adj[0]), _ptr(adj[1]),
                                    _ptr(adj[2]), _ptr(adj[3]), _ptr(adj[4]), _ptr(adj[5]), C.c_int32(pol), (C.c_float * 3)(*origin),
                                    C.c_double(scale), _ptr(flip), _ptr(face_comp), _ptr(faces_out), _ptr(comp_faces),
                                    _ptr(comp_flags), _ptr(vol_hi), _ptr(vol_lo), _ptr(counts), _ptr(scratch),
                                    C.c_size_t(scratch.numel()), _stream()), "arah_mesh_orient")
    return flip, face_comp, faces_out, comp_faces, comp_flags, vol_hi, vol_lo, counts


def mesh_intersections(verts, faces, group=None, between=False, quant=None, max_pairs=1 << 20, want_tested=False, trim=True):
    """Which faces of an indexed mesh cut through each other (arah_mesh_intersections, csrc/meshintersect.hpp): verts (V,3) float32
    and faces (F,3) integer ids on the GPU, group (F,) uint8 or None, between: only pairs from different groups count.  -> hits (F,)
    int32, vert_hit (V,) uint8, pair_start (F+1,) int32, pairs (n,2) int32, counts (5,) int32 as meshing.mesh_intersections describes
    them, and equal to it bit for bit; with want_tested a sixth result, the (1,) int64 number of pairs that reached the six tests.
    One host read for the vertices' bounds (meshing.orient_quant) unless `quant` is given.  trim=True reads the pair total once
    more, to return pairs with its n = counts[4] rows and to raise ValueError for more than 2^31 - 1 pairs; trim=False returns the
    (max_pairs, 2) buffer, zero from row counts[4] on, without that read -- counts[0] == -1 then says that the pairs did not fit."""
    from . import meshing
    require_gpu()
    lib = load_library()
    what = "mesh_intersections"
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("%s: verts must be a (V, 3) float32 tensor" % what)
    f, V, F = _mesh_cc_args(faces, int(verts.shape[0]), what)
    v = verts.detach().contiguous()
    if v.device != f.device:
        raise ValueError("%s: verts live on %s, faces on %s" % (what, v.device, f.device))
    if F > meshing.INTERSECT_MAX_FACES:
        raise ValueError("%s: at most 2^26 faces, got %d" % (what, F))
    between = meshing.check_between(between, group, what)
    group = meshing.check_group(group, F, f.device, what)
    cap = meshing.check_max_pairs(max_pairs, what)
    origin, scale = meshing._check_quant(meshing.orient_quant(v) if quant is None else quant, what)
    dev, i32 = f.device, torch.int32
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_intersections_scratch_bytes(V, F, cap)))
        hits = torch.empty(F, dtype=i32, device=dev)
        vert_hit = torch.empty(V, dtype=torch.uint8, device=dev)
        pair_start = torch.empty(F + 1, dtype=i32, device=dev)
        pairs = torch.empty(cap, 2, dtype=i32, device=dev)
        counts = torch.empty(5, dtype=i32, device=dev)
        tested = torch.empty(1, dtype=torch.int64, device=dev) if want_tested else None
        _check(lib.arah_mesh_intersections(_ptr(v), C.c_int64(V), _ptr(f), C.c_int64(F), _ptr(group.contiguous()) if between else None,
                                           C.c_int32(1 if between else 0), (C.c_float * 3)(*origin), C.c_double(scale), C.c_int64(cap),
                                           _ptr(hits), _ptr(vert_hit), _ptr(pair_start), _ptr(pairs) if cap else None, _ptr(counts),
                                           _ptr(tested), _ptr(scratch), C.c_size_t(scratch.numel()), _stream()),
               "arah_mesh_intersections")
    if trim:
        total, _, _, _, written = counts.tolist()
        if total < 0:
            raise ValueError("%s: more than 2^31 - 1 pairs do not fit an int32 count" % what)
        pairs = pairs[:written]
    return (hits, vert_hit, pair_start, pairs, counts) + ((tested,) if want_tested else ())


def mesh_boundary_loops(faces, n_verts, adjacency=None):
    """Boundary half-edges and loops of an indexed mesh (arah_mesh_boundary_loops): faces (F,3) integer ids on the GPU over n_verts
    vertices, adjacency: `mesh_adjacency` of them, or None to build it here.  -> edges (3F,2), edge_face, edge_loop (3F,) int32,
    loop_edges (V,) int32, loop_simple (V,) uint8, loop_vert (V,) int32, counts (3,) int32 as meshing.mesh_boundary_loops describes
    them, and equal to it bit for bit.  All on the device, no host synchronisation."""
    require_gpu()
    lib = load_library()
    f, V, F, adj = _mesh_adj_only(faces, n_verts, adjacency, "mesh_boundary_loops")
    dev, i32 = f.device, torch.int32
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_boundary_loops_scratch_bytes(V, F)))
        edges = torch.empty(3 * F, 2, dtype=i32, device=dev)
        edge_face, edge_loop = (torch.empty(3 * F, dtype=i32, device=dev) for _ in range(2))
        loop_edges, loop_vert = (torch.empty(V, dtype=i32, device=dev) for _ in range(2))
        loop_simple = torch.empty(V, dtype=torch.uint8, device=dev)
        counts = torch.empty(3, dtype=i32, device=dev)
        _check(lib.arah_mesh_boundary_loops(_ptr(f), C.c_int64(F), C.c_int64(V), _ptr(adj[2]), _ptr(adj[3]), _ptr(adj[4]), _ptr(adj[5]),
                                            _ptr(edges), _ptr(edge_face), _ptr(edge_loop), _ptr(loop_edges), _ptr(loop_simple),
                                            _ptr(loop_vert), _ptr(counts), _ptr(scratch), C.c_size_t(scratch.numel()), _stream()),
               "arah_mesh_boundary_loops")
    return edges, edge_face, edge_loop, loop_edges, loop_simple, loop_vert, counts


def mesh_fill_holes(verts, faces, max_edges=64, adjacency=None, loops=None, quant=None):
    """Small holes closed by a fan (arah_mesh_fill_holes): verts (V,3) float32 and faces (F,3) integer ids on the GPU, loops: the
    arrays of `mesh_boundary_loops` of the mesh, or None to build them here (from `adjacency`, itself built when None).  ->
    verts_out (V + V // 3, 3) float32, vert_src (V + V // 3,) int32, faces_out (4F,3) int32, face_loop (4F,) int32, counts (5,)
    int32 as meshing.mesh_fill_holes describes them, and equal to it bit for bit.  One host synchronisation: the vertices' bounds
    (meshing.fill_quant), none when `quant` is given."""
    from . import meshing
    require_gpu()
    lib = load_library()
    max_edges = meshing.check_max_edges(max_edges)
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("mesh_fill_holes: verts must be a (V, 3) float32 tensor")
    V = int(verts.shape[0])
    f, _, F = _mesh_cc_args(faces, V, "mesh_fill_holes")
    if verts.device != f.device:
        raise ValueError("mesh_fill_holes: verts live on %s, faces on %s" % (verts.device, f.device))
    if F > meshing.ADJACENCY_MAX_FACES:
        raise ValueError("mesh_fill_holes: at most 2^28 faces, got %d" % F)
    v = verts.detach().contiguous()
    origin, scale = meshing._check_quant(meshing.fill_quant(v) if quant is None else quant, "mesh_fill_holes")
    if loops is None:
        loops = mesh_boundary_loops(f, V, adjacency=adjacency)
    else:
        loops = tuple(loops)
        shapes = ((3 * F, 2), (3 * F,), (3 * F,), (V,), (V,), (V,), (3,))
        if len(loops) != 7 or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != s or t.device != f.device
                                  or t.dtype != (torch.uint8 if i == 4 else torch.int32)
                                  for i, (t, s) in enumerate(zip(loops, shapes))):
            raise ValueError("mesh_fill_holes: loops must be the seven arrays of mesh_boundary_loops of this mesh, on %s" % (f.device,))
        loops = tuple(t.contiguous() for t in loops)
    dev, i32 = f.device, torch.int32
    with _on_device(dev):
        scratch = _mesh_cc_buf(dev, int(lib.arah_mesh_fill_holes_scratch_bytes(V, F)))
        verts_out = torch.empty(V + V // 3, 3, dtype=torch.float32, device=dev)
        vert_src = torch.empty(V + V // 3, dtype=i32, device=dev)
        faces_out = torch.empty(4 * F, 3, dtype=i32, device=dev)
        face_loop = torch.empty(4 * F, dtype=i32, device=dev)
        counts = torch.empty(5, dtype=i32, device=dev)
        _check(lib.arah_mesh_fill_holes(_ptr(v), C.c_int64(V), _ptr(f), C.c_int64(F), _ptr(loops[0]), _ptr(loops[2]), _ptr(loops[3]),
                                        _ptr(loops[4]), _ptr(loops[5]), _ptr(loops[6]), C.c_int32(max_edges), (C.c_float * 3)(*origin),
                                        C.c_double(scale), _ptr(verts_out), _ptr(vert_src), _ptr(faces_out), _ptr(face_loop),
                                        _ptr(counts), _ptr(scratch), C.c_size_t(scratch.numel()), _stream()), "arah_mesh_fill_holes")
    return verts_out, vert_src, faces_out, face_loop, counts


def mesh_rasterize(verts_uvz, faces, height, width, z_near=1e-4, cull="none", thresholds=None):
    """An indexed mesh drawn on the device (arah_mesh_rasterize, csrc/meshraster.hpp): verts_uvz (V,3) float32 (u, v, view depth) and
    faces (F,3) integer ids on the GPU -> pix_to_face (H,W) int32, depth (H,W) float32, bary (H,W,3) float32, -1 where nothing
    covers; meshing.mesh_rasterize bit for bit.  The key buffer is allocated here and initialised inside the call; no host
    synchronisation.  thresholds: (small_area, wave_area, huge_area) of pass A instead of the built-in ones
    (arah_mesh_rasterize_debug; the image is the same for every choice), for measuring them."""
    from . import meshing
    require_gpu()
    lib = load_library()
    verts, H, W, cull_code = meshing.check_raster_args(verts_uvz, faces, height, width, cull)
    V = int(verts.shape[0])
    f, _, F = _mesh_cc_args(faces, V, "mesh_rasterize")
    v = verts.contiguous()
    dev = v.device
    with _on_device(dev):
        keys = torch.empty(H * W, dtype=torch.int64, device=dev)
        pix_to_face = torch.empty(H, W, dtype=torch.int32, device=dev)
        depth = torch.empty(H, W, dtype=torch.float32, device=dev)
        bary = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
        head = (_ptr(v) if V else None, C.c_int64(V), _ptr(f) if F else None, C.c_int64(F), C.c_int32(H), C.c_int32(W),
                C.c_float(float(z_near)), C.c_int32(cull_code))
        tail = (_ptr(keys), _ptr(pix_to_face), _ptr(depth), _ptr(bary), _stream())
        if thresholds is None:
            _check(lib.arah_mesh_rasterize(*head, *tail), "arah_mesh_rasterize")
        else:
            _check(lib.arah_mesh_rasterize_debug(*head, *(C.c_int32(int(t)) for t in tuple(thresholds)[:3]), *tail),
                   "arah_mesh_rasterize_debug")
    return pix_to_face, depth, bary


def mesh_interpolate(pix_to_face, bary, faces, attr, background=0.0):
    """Per-vertex attributes attr (V,C) float32, 1 <= C <= 32, drawn with the pix_to_face (H,W) and bary (H,W,3) of `mesh_rasterize`
    (arah_mesh_interpolate), all on the GPU: -> (H,W,C) float32, `background` where no face was drawn;
    meshing.interpolate_attributes bit for bit.  A gather per pixel and channel; no host synchronisation."""
    from . import meshing
    require_gpu()
    lib = load_library()
    p2f, b, a = meshing.check_interpolate_args(pix_to_face, bary, faces, attr, "mesh_interpolate")
    V, Cn = int(a.shape[0]), int(a.shape[1])
    f, _, F = _mesh_cc_args(faces, V, "mesh_interpolate")
    H, W = int(p2f.shape[0]), int(p2f.shape[1])
    if H * W > 2 ** 31 - 1:
        raise ValueError("mesh_interpolate: at most 2^31 - 1 pixels")
    dev = a.device
    if p2f.dtype != torch.int32:   # ids that do not fit int32 name no face: -1
        p2f = p2f.long()
        p2f = torch.where((p2f >= 0) & (p2f <= 2 ** 31 - 1), p2f, torch.full_like(p2f, -1)).to(torch.int32)
    p2f, b, a = p2f.contiguous(), b.contiguous(), a.contiguous()
    with _on_device(dev):
        out = torch.empty(H, W, Cn, dtype=torch.float32, device=dev)
        _check(lib.arah_mesh_interpolate(_ptr(p2f), _ptr(b), C.c_int32(H), C.c_int32(W), _ptr(f) if F else None, C.c_int64(F),
                                         _ptr(a) if V else None, C.c_int64(V), C.c_int32(Cn), C.c_float(float(background)),
                                         _ptr(out), _stream()), "arah_mesh_interpolate")
    return out


def marching_cubes(sdf, level=0.0, cap=1 << 20):
    """Level set of the lattice volume sdf (N,N,N) [ix,iy,iz] as a triangle soup, on the device and WITHOUT a host round
    trip: -> tris (cap,3,3) coordinates in [-1,1]^3 (rows beyond the count are zero: degenerate triangles), n_tris (1,) int32
    on the device (the size of the level set; it may exceed cap, then only the first cap triangles were written).  The case
    table is meshing.case_table(), copied to the device once; the result is meshing.marching_cubes(sdf) triangle for triangle."""
    require_gpu()
    lib = load_library()
    v = _f32(sdf)
    if v.dim() != 3 or v.shape[0] != v.shape[1] or v.shape[0] != v.shape[2] or v.shape[0] < 2:
        raise ValueError("sdf must be an (N, N, N) lattice volume")
    dev, N = v.device, int(v.shape[0])
    table, ntri = _mc_device_tables(dev)
    with _on_device(dev):
        tris = torch.empty(int(cap), 3, 3, device=dev)
        n_tris = torch.empty(1, dtype=torch.int32, device=dev)
        scratch = torch.empty(int(lib.arah_marching_cubes_scratch_bytes(N)), dtype=torch.uint8, device=dev)
        _check(lib.arah_marching_cubes(_ptr(v), C.c_int32(N), C.c_float(float(level)), _ptr(table), _ptr(ntri), _ptr(tris),
                                       C.c_int32(int(cap)), _ptr(n_tris), _ptr(scratch), C.c_size_t(scratch.numel()), _stream()),
               "arah_marching_cubes")
    return tris, n_tris


METRICS_STATUS = {0: "ok", 1: "the frame's ray mask is empty",
                  2: "the mask's bounding rectangle is narrower or lower than the 7 x 7 SSIM window"}


def image_metrics(pred, gt, box_mask, data_range=2.0):
    """PSNR and SSIM of a rendered frame against its ground truth (im2mesh/utils/eval.py:6-18) on the device, in float64 and
    WITHOUT a host round trip (arah_image_metrics): pred / gt (H,W,3) float images, box_mask (H,W) bool / uint8, non-zero = the
    frame's rays (the reference's `mask_at_box`: PSNR over those pixels, SSIM on their bounding rectangle).  data_range: R of
    C1 = (0.01 R)^2, C2 = (0.03 R)^2; 2.0 is what scikit-image 0.18.1 takes for float images, pass 1.0 to compare against a
    call with data_range=1.  -> out (4,) float64 on the device: psnr, ssim, mse, number of masked pixels; rect (5,) int32: x, y,
    w, h, status (METRICS_STATUS).  Nothing is checked here: `read_image_metrics` raises for a status != 0 when the result is
    read.  Bit-reproducible: no atomics, fixed summation order."""
    require_gpu()
    lib = load_library()
    dev = _same_device(pred, gt, box_mask)
    p, g = _f32(pred), _f32(gt)
    if p.dim() != 3 or p.shape[2] != 3 or g.shape != p.shape or tuple(box_mask.shape) != tuple(p.shape[:2]):
        raise ValueError("pred, gt must be (H, W, 3) images of one size and box_mask (H, W)")
    if not float(data_range) > 0.0:
        raise ValueError("data_range must be positive")
    m = box_mask.detach().contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)
    H, W = int(p.shape[0]), int(p.shape[1])
    with _on_device(dev):
        out = torch.empty(4, dtype=torch.float64, device=dev)
        rect = torch.empty(5, dtype=torch.int32, device=dev)
        scratch = torch.empty(int(lib.arah_image_metrics_bytes(H, W)), dtype=torch.uint8, device=dev)
        _check(lib.arah_image_metrics(_ptr(p), _ptr(g), _ptr(m), C.c_int32(H), C.c_int32(W), C.c_double(float(data_range)),
                                      _ptr(out), _ptr(rect), _ptr(scratch), C.c_size_t(scratch.numel()), _stream()),
               "arah_image_metrics")
    return out, rect


def read_image_metrics(out, rect, what="the frame"):
    """Host values of an `image_metrics` result (this is where the stream is waited for): {"psnr", "ssim", "mse", "n", "rect"}.
    Raises ValueError, as scikit-image does for such a crop, when the status says that no SSIM exists."""
    o, r = out.detach().cpu().tolist(), rect.detach().cpu().tolist()
    if r[4] != 0:
        raise ValueError("no SSIM for %s: %s (rectangle x %d y %d w %d h %d)" % (what, METRICS_STATUS.get(r[4], r[4]), *r[:4]))
    return {"psnr": o[0], "ssim": o[1], "mse": o[2], "n": int(o[3]), "rect": tuple(r[:4])}


@_guarded
def skin_lbs_counted(frame, ws, x_hat, n_items, per_item=1):
    """Forward skinning of the first n_items[0] * per_item rows of x_hat (P,3) -- a count that lives on the device -- ->
    x_bar (P,3), zero beyond.  (The vertices of a mesh hip.marching_cubes just extracted, per_item = 3.)"""
    lib = load_library()
    x = _f32(x_hat)
    buf = ws.ensure(1, 1)
    xb = torch.zeros(x.shape[0], 3, device=x.device)
    _check(lib.arah_skin_lbs_counted(C.byref(frame.handle), _ptr(x), C.c_int32(int(x.shape[0])), _ptr(n_items),
                                     C.c_int32(int(per_item)), _ptr(xb), _ptr(buf), C.c_size_t(buf.numel()), _stream()),
           "arah_skin_lbs_counted")
    return xb


def gemv_rows(weight, x, b0=None, b1=None):
    """y = weight @ x + b0 + b1 for ONE vector x (the wide output layers of the hypernetwork, an HBM stream of `weight`);
    no autograd.  weight (R, C) fp32 contiguous, C % 4 == 0."""
    require_gpu()
    lib = load_library()
    w, xv = weight.detach(), _f32(x).reshape(-1)
    if not (w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 2 and w.shape[1] == xv.numel() and w.shape[1] % 4 == 0):
        raise ValueError("gemv_rows: weight (R, C) fp32 contiguous with C % 4 == 0 and x of C elements")
    with _on_device(w.device):
        y = torch.empty(w.shape[0], device=w.device)
        _check(lib.arah_gemv_rows(_ptr(w), C.c_int32(w.shape[0]), C.c_int32(w.shape[1]), _ptr(xv),
                                  _ptr(None if b0 is None else _f32(b0).reshape(-1)),
                                  _ptr(None if b1 is None else _f32(b1).reshape(-1)), _ptr(y), _stream()), "arah_gemv_rows")
    return y


def rasterize(tri_uvz, height, width, z_near=1e-4):
    """tri_uvz (F,3,3) pixel-space corners (u, v, view depth) -> pix_to_face (H,W) int64, -1 where nothing covers."""
    require_gpu()
    lib = load_library()
    tri = _f32(tri_uvz)
    dev = tri.device
    with _on_device(dev):
        zbuf = torch.full((height * width,), -1, dtype=torch.int64, device=dev)   # all bits set
        _check(lib.arah_rasterize(_ptr(tri), C.c_int32(int(tri.shape[0])), C.c_int32(int(height)), C.c_int32(int(width)),
                                  C.c_float(float(z_near)), _ptr(zbuf), _stream()), "arah_rasterize")
    face = (zbuf & 0xffffffff).reshape(height, width)
    return torch.where(zbuf.reshape(height, width) == -1, torch.full_like(face, -1), face)


@_guarded
def skin_lbs(frame, ws, x_hat):
    lib = load_library()
    x = _f32(x_hat)
    n = x.shape[0]
    buf = ws.ensure(1, 1)
    w = torch.empty(n, 24, device=x.device)
    xb = torch.empty(n, 3, device=x.device)
    T = torch.empty(n, 4, 4, device=x.device)
    _check(lib.arah_skin_lbs(C.byref(frame.handle), _ptr(x), C.c_int32(n), _ptr(w), _ptr(xb), _ptr(T), _ptr(buf),
                             C.c_size_t(buf.numel()), _stream()), "arah_skin_lbs")
    return w, xb, T


@_guarded
def skin_jacobian(frame, ws, x_hat):
    lib = load_library()
    x = _f32(x_hat)
    n = x.shape[0]
    buf = ws.ensure(1, 1)
    jac = torch.empty(n, 3, 3, device=x.device)
    _check(lib.arah_skin_jacobian(C.byref(frame.handle), _ptr(x), C.c_int32(n), _ptr(jac), _ptr(buf),
                                  C.c_size_t(buf.numel()), _stream()), "arah_skin_jacobian")
    return jac


@_guarded
def color_eval(frame, ws, x_norm, normal, view, feat):
    lib = load_library()
    x, nr, ft = _f32(x_norm), _f32(normal), _f32(feat)
    vw = _f32(view) if view is not None else None
    n = x.shape[0]
    buf = ws.ensure(1, 1)
    rgb = torch.empty(n, 3, device=x.device)
    _check(lib.arah_color_eval(C.byref(frame.handle), _ptr(x), _ptr(nr), _ptr(vw), _ptr(ft), C.c_int32(n), _ptr(rgb),
                               _ptr(buf), C.c_size_t(buf.numel()), _stream()), "arah_color_eval")
    return rgb


@_guarded
def shade_points(frame, ws, x_norm, T, dirs, cano_view_dirs=True, shade_engine=None):
    """The per-sample half of loop D on the frame's own engine (arah_shade_points): n normalised canonical points with their
    transforms (n,4,4) and ray directions (n,3) -> rgb (n,3), density (n,), sdf (n,), d sdf / d x_norm (n,3)."""
    lib = load_library()
    x, Tm, d = _f32(x_norm), _f32(T), _f32(dirs)
    n = x.shape[0]
    buf = ws.ensure(n, 1)
    rgbs = torch.empty(n, 4, device=x.device)
    sdfn = torch.empty(n, 4, device=x.device)
    eng = default_shade_engine() if shade_engine is None else int(shade_engine)
    _check(lib.arah_shade_points(C.byref(frame.handle), _ptr(x), _ptr(Tm), _ptr(d), C.c_int32(n), C.c_int32(int(bool(cano_view_dirs))),
                                 C.c_int32(eng), _ptr(rgbs), _ptr(sdfn), _ptr(buf), C.c_size_t(buf.numel()), _stream()), "arah_shade_points")
    return rgbs[:, :3], rgbs[:, 3], sdfn[:, 0], sdfn[:, 1:]


def sample_depths_debug(variant, sampling, near_far, conv, start, end):
    """Tests: (z [N,S] float32, mask [N,S] uint8), the eval-mode depth samples of N rays by the serial kernel (variant 0) or the
    wave-per-ray one (variant 1); `sampling` is a Sampling (its n_steps / n_near / n_far and linspace tables)."""
    dev = near_far.device
    nf, st, en = _f32(near_far), _f32(start), _f32(end)
    cv = conv.to(torch.uint8).contiguous()
    n, S = int(st.shape[0]), int(sampling.n_steps)
    z = torch.empty(n, S, device=dev)
    mask = torch.empty(n, S, dtype=torch.uint8, device=dev)
    with _on_device(dev):
        _check(load_library().arah_sample_depths_debug(
            C.c_int32(int(variant)), C.c_int32(n), C.c_int32(S), C.c_int32(int(sampling.n_near)), C.c_int32(int(sampling.n_far)),
            _ptr(nf), _ptr(cv), _ptr(st), _ptr(en), _ptr(sampling.lin_steps), _ptr(sampling.lin_near), _ptr(sampling.lin_far),
            _ptr(z), _ptr(mask), _stream(dev)), "arah_sample_depths_debug")
    return z, mask


# byte offsets of a body buffer's arrays (include/arah_hip.h: ARAH_BODY_OFF_*)
BODY_OFF_SPHERES, BODY_OFF_GRID, BODY_OFF_CELLS, BODY_CELL_BYTES = 114688, 118784, 119040, 64


def cell_clusters_debug(variant, body_buf):
    """Tests: the candidate lists [n_cells, 64] uint8 of the grid and cluster spheres held in `body_buf` (BodyTables.buf), rebuilt
    by the serial kernel (variant 0) or the wave-per-cell one (variant 1) into a buffer of their own."""
    dev = body_buf.device
    n_cells = int(body_buf[BODY_OFF_GRID:BODY_OFF_GRID + 48].view(torch.int32)[8].item())
    cells = torch.zeros(n_cells, BODY_CELL_BYTES, dtype=torch.uint8, device=dev)
    with _on_device(dev):
        _check(load_library().arah_cell_clusters_debug(C.c_int32(int(variant)), _ptr(body_buf[BODY_OFF_GRID:]),
                                                       _ptr(body_buf[BODY_OFF_SPHERES:]), _ptr(cells), _stream(dev)),
               "arah_cell_clusters_debug")
    return cells


@_guarded
def nearest_inverse_lbs(frame, ws, pts):
    lib = load_library()
    p = _f32(pts)
    n = p.shape[0]
    buf = ws.ensure(1, 1)
    idx = torch.empty(n, dtype=torch.int32, device=p.device)
    x0 = torch.empty(n, 3, device=p.device)
    T0 = torch.empty(n, 4, 4, device=p.device)
    _check(lib.arah_nearest_inverse_lbs(C.byref(frame.handle), _ptr(p), C.c_int32(n), _ptr(idx), _ptr(x0), _ptr(T0),
                                        _ptr(buf), C.c_size_t(buf.numel()), _stream()), "arah_nearest_inverse_lbs")
    return idx, x0, T0


@_guarded
def broyden3_lbs(frame, ws, tgt, x0, T0, canon_kernel=None):
    lib = load_library()
    kern = default_canon_kernel() if canon_kernel is None else int(canon_kernel)
    tgt, x0, T0 = _f32(tgt), _f32(x0), _f32(T0)
    n = tgt.shape[0]
    buf = ws.ensure(n, 1)
    x = torch.empty(n, 3, device=tgt.device)
    T = torch.empty(n, 4, 4, device=tgt.device)
    err = torch.empty(n, device=tgt.device)
    conv = torch.empty(n, dtype=torch.uint8, device=tgt.device)
    _check(lib.arah_broyden3_lbs(C.byref(frame.handle), _ptr(tgt), _ptr(x0), _ptr(T0), C.c_int32(n), _ptr(x), _ptr(T),
                                 _ptr(err), _ptr(conv), C.c_int32(kern), _ptr(buf), C.c_size_t(buf.numel()), _stream()),
           "arah_broyden3_lbs")
    return x, T, err, conv.bool()


@_guarded
def joint_root_find(frame, ws, cam_loc, dirs, valid, x0, z0, T0):
    """Loop B on caller-supplied starts: cam_loc (B,3), dirs (N,3), valid (N,) bool/uint8, x0 (N,3) raw canonical,
    z0 (N,), T0 (N,4,4) -> x, z, T, conv."""
    lib = load_library()
    cam, d, x0, z0, T0 = _f32(cam_loc), _f32(dirs), _f32(x0), _f32(z0), _f32(T0)
    v = valid.to(torch.uint8).contiguous()
    n = d.shape[0]
    buf = ws.ensure(n, 1)
    dev = d.device
    x = torch.empty(n, 3, device=dev)
    z = torch.empty(n, device=dev)
    T = torch.empty(n, 4, 4, device=dev)
    conv = torch.empty(n, dtype=torch.uint8, device=dev)
    _check(lib.arah_joint_root_find(C.byref(frame.handle), _ptr(cam), C.c_int32(n // cam.shape[0]), _ptr(d), _ptr(v),
                                    _ptr(x0), _ptr(z0), _ptr(T0), C.c_int32(n), _ptr(x), _ptr(z), _ptr(T), _ptr(conv),
                                    _ptr(buf), C.c_size_t(buf.numel()), _stream()), "arah_joint_root_find")
    return x, z, T, conv.bool()


@_guarded
def trace(frame, ws, cam_loc, dirs, near_far, root_find_all=False):
    """cam_loc (B,3), dirs (B*N,3) flat, near_far (B*N,2) -> x_norm, T, conv, start, end."""
    lib = load_library()
    cam, d, nf = _f32(cam_loc), _f32(dirs), _f32(near_far)
    n = d.shape[0]
    buf = ws.ensure(n, 1)
    dev = d.device
    xn = torch.empty(n, 3, device=dev)
    T = torch.empty(n, 4, 4, device=dev)
    conv = torch.empty(n, dtype=torch.uint8, device=dev)
    start = torch.empty(n, device=dev)
    end = torch.empty(n, device=dev)
    _check(lib.arah_trace(C.byref(frame.handle), _ptr(cam), C.c_int32(n // cam.shape[0]), _ptr(d), _ptr(nf),
                          C.c_int32(n), C.c_int32(int(bool(root_find_all))), _ptr(xn), _ptr(T), _ptr(conv), _ptr(start),
                          _ptr(end), _ptr(buf), C.c_size_t(buf.numel()), _stream()), "arah_trace")
    return xn, T, conv, start, end


@_guarded
def sample_canonicalize(frame, ws, sampling, cam_loc, dirs, near_far, conv, start, end, rand=None):
    """rand: None (eval) or (rand_steps (N,S), rand_near (N,near+1), rand_far (N,far)) uniform draws."""
    lib = load_library()
    r_s = r_n = r_f = None
    if rand is not None:
        r_s, r_n, r_f = [_f32(t) for t in rand]
    cam, d, nf = _f32(cam_loc), _f32(dirs), _f32(near_far)
    n, S = d.shape[0], sampling.n_steps
    buf = ws.ensure(n, S)
    dev = d.device
    z = torch.empty(n, S, device=dev)
    pts = torch.empty(n, S, 3, device=dev)
    T = torch.empty(n, S, 4, 4, device=dev)
    mask = torch.empty(n, S, dtype=torch.uint8, device=dev)
    _check(lib.arah_sample_canonicalize(C.byref(frame.handle), C.byref(sampling.handle), _ptr(cam),
                                        C.c_int32(n // cam.shape[0]), _ptr(d), _ptr(nf), _ptr(conv.contiguous()),
                                        _ptr(_f32(start)), _ptr(_f32(end)), C.c_int32(n), _ptr(r_s), _ptr(r_n), _ptr(r_f),
                                        _ptr(z), _ptr(pts), _ptr(T), _ptr(mask), _ptr(buf), C.c_size_t(buf.numel()),
                                        _stream()),
           "arah_sample_canonicalize")
    return z, pts, T, mask


@_guarded
def shade_composite(frame, ws, sampling, dirs, z, pts, T, mask):
    lib = load_library()
    d = _f32(dirs)
    n, S = d.shape[0], sampling.n_steps
    buf = ws.ensure(n, S)
    dev = d.device
    rgb = torch.empty(n, 3, device=dev)
    acc = torch.empty(n, device=dev)
    vol = torch.empty(n, dtype=torch.uint8, device=dev)
    _check(lib.arah_shade_composite(C.byref(frame.handle), C.byref(sampling.handle), _ptr(d), _ptr(_f32(z)),
                                    _ptr(_f32(pts)), _ptr(_f32(T)), _ptr(mask.contiguous()), C.c_int32(n), _ptr(rgb),
                                    _ptr(acc), _ptr(vol), _ptr(buf), C.c_size_t(buf.numel()), _stream()),
           "arah_shade_composite")
    return rgb, acc, vol


# ------------------------------------------------------------------------------------------------
# loop D with gradients: the pair of entry points behind training.ShadeSamples (torch.autograd.Function)
# ------------------------------------------------------------------------------------------------
KIN_PAD = {COLOR_NO_VIEW_DIR: 272, COLOR_IDR: 304}   # colour input [feat(256) | x(3) | n(3) | PE(view)(27)] padded to 16


def _grouped(groups, n, width, device, inner=None):
    """(groups[, inner], roundup(n, 64), width) floats whose padding rows are zero: the operand streams of products over the sample
    axis that travel together (see tall.gram_grouped).  The kernels write rows [0, n) of each slice."""
    # a step's sample count moves by a few hundred from frame to frame: rounded up to 8192 / 2048 rows the gigabyte-sized groups
    # come in one or two sizes and torch's allocator hands the same blocks out again (rounded to 64 only, every other step of
    # bench.py's training line paid a 35 ms device allocation)
    n_pad = (n + 8191) // 8192 * 8192 if n >= 65536 else ((n + 2047) // 2048 * 2048 if n >= 16384 else (n + 63) // 64 * 64)
    shape = (groups, n_pad, width) if inner is None else (groups, inner, n_pad, width)
    buf = torch.empty(*shape, device=device)
    if n_pad > n:
        buf[..., n:, :].zero_()
    return buf


def _train_in(x, T, view, view_orig, rotate_normal, ray_augm, g_s=None, g_rgb=None):
    t = ArahTrainIn()
    t.n, t.rotate_normal, t.ray_augm = int(x.shape[0]), int(bool(rotate_normal)), int(bool(ray_augm))
    t.x, t.T, t.view, t.view_orig = _ptr(x), _ptr(T), _ptr(view), _ptr(view_orig)
    t.g_s, t.g_rgb = _ptr(g_s), _ptr(g_rgb)
    return t


@_guarded
def shade_train_forward(frame, ws, x, T, view, view_orig, rotate_normal, ray_augm, keep=False):
    """x (P,3) normalised canonical points, T (P,4,4) or None, view / view_orig (P,3) -> sdf (P,), rgb (P,3).
    keep=True: also the hand-over for shade_train_backward -- dict(cin, c, rgb4): the colour MLP's input and hidden
    activations as (P, width) streams and the padded rgb; the backward then skips the normal sweep and the colour MLP."""
    lib = load_library()
    x, view = _f32(x), _f32(view)
    T = _f32(T) if (T is not None and rotate_normal) else None
    vo = _f32(view_orig) if (view_orig is not None and ray_augm) else None
    n = x.shape[0]
    buf = ws.ensure(1, 1)
    sdf = torch.empty(n, device=x.device)
    rgb4 = torch.empty(n, 4, device=x.device)
    tin = _train_in(x, T, view, vo, rotate_normal, ray_augm)
    kept = None
    if keep:
        # the 256-wide activations sit next to each other, padded to a multiple of 64 rows with zeros: the weight-gradient
        # products of the backward then run as ONE batched split-K product per group (tall.gram_grouped), all views
        cc = _grouped(4, n, 256, x.device)
        cinp, c2p = _grouped(1, n, KIN_PAD[frame.color_mode], x.device)[0], _grouped(1, n, 128, x.device)[0]
        kept = {"cin": cinp[:n], "c": [cc[0, :n], cc[2, :n], c2p[:n], cc[1, :n], cc[3, :n]], "rgb4": rgb4, "cc": cc,
                "cin_pad": cinp, "c2_pad": c2p}
        tin.tap_cin = _ptr(kept["cin"])
        for i, t in enumerate(kept["c"]):
            tin.tap_c[i] = _ptr(t).value
    _check(lib.arah_shade_train_forward(C.byref(frame.handle), C.byref(tin), _ptr(sdf), _ptr(rgb4), _ptr(buf),
                                        C.c_size_t(buf.numel()), _stream()), "arah_shade_train_forward")
    return (sdf, rgb4[:, :3], kept) if keep else (sdf, rgb4[:, :3])


def _sdf_streams(n, dev):
    """Operand streams of the SIREN's weight gradients, grouped for tall.gram_grouped: `avv` (6, 2, n_pad, 256) holds adj v_k and
    adj vd_k of layer k next to each other, `hh` (5, 2, n_pad, 256) their partners h_k and hd_k (k = 1..5), `h0` (2, n_pad, 4) the
    first layer's h_0 = x and hd_0 = nt.  dW_k = adj(v_k)^T h_{k-1} + adj(vd_k)^T hd_{k-1} is then ONE product over 2 n_pad rows."""
    avv, hh, h0 = _grouped(6, n, 256, dev, inner=2), _grouped(5, n, 256, dev, inner=2), _grouped(2, n, 4, dev)
    return {"h": [h0[0, :n]] + [hh[k, 0, :n] for k in range(5)],
            "hd": [h0[1, :n]] + [hh[k, 1, :n] for k in range(5)] + [torch.empty(n, 256, device=dev)],
            "av": [avv[k, 0, :n] for k in range(6)], "avd": [avv[k, 1, :n] for k in range(6)], "avv": avv, "hh": hh, "h0": h0}


@_guarded
def sdf_normal_forward(frame, ws, x):
    """The regulariser queries (IDR:104-128): x (P,3) normalised canonical points -> sdf (P,) in normalised units and its
    gradient d sdf / d x (P,3), by the training kernel without its colour half (ArahTrainIn.geom_only)."""
    lib = load_library()
    x = _f32(x)
    n = x.shape[0]
    buf = ws.ensure(1, 1)
    sdf = torch.empty(n, device=x.device)
    n4 = torch.empty(n, 4, device=x.device)
    tin = _train_in(x, None, None, None, False, False)
    tin.geom_only = 1
    _check(lib.arah_shade_train_forward(C.byref(frame.handle), C.byref(tin), _ptr(sdf), _ptr(n4), _ptr(buf),
                                        C.c_size_t(buf.numel()), _stream()), "arah_shade_train_forward")
    return sdf, n4[:, :3]


@_guarded
def sdf_normal_backward(frame, ws, x, g_s, g_n):
    """dL/dx (P,3) and the operand streams of the SDF weight gradients (h, hd, av, avd, the feature h_6 as `feat`,
    film_freq, film_phase) for upstream gradients g_s (P,) on the value and g_n (P,3) on the normal."""
    lib = load_library()
    x, g_s, g_n = _f32(x), _f32(g_s), _f32(g_n)
    n, dev = x.shape[0], x.device
    buf = ws.ensure(1, 1)
    E = lambda *shape: torch.empty(*shape, device=dev)
    st = {"gx4": E(n, 4), "film_freq": E(6, 256), "film_phase": E(6, 256), "feat": E(n, 256)}
    st.update(_sdf_streams(n, dev))
    g = ArahTrainGrads()
    for k in ("gx4", "film_freq", "film_phase"):
        setattr(g, k, _ptr(st[k]))
    for k in ("h", "hd", "av", "avd"):
        arr = getattr(g, k)
        for i, t in enumerate(st[k]):
            arr[i] = _ptr(t).value
    g.c[0] = _ptr(st["feat"]).value
    nslab = lib.arah_shade_train_slab_bytes()
    if getattr(ws, "train_slab", None) is None or ws.train_slab.numel() < nslab:
        ws.train_slab = torch.empty(nslab, dtype=torch.uint8, device=dev)
    tin = _train_in(x, None, None, None, False, False, g_s, g_n)
    tin.geom_only = 1
    _check(lib.arah_shade_train_backward(C.byref(frame.handle), C.byref(tin), C.byref(g), _ptr(ws.train_slab),
                                         C.c_size_t(ws.train_slab.numel()), _ptr(buf), C.c_size_t(buf.numel()),
                                         _stream()), "arah_shade_train_backward")
    return st


@_guarded
def shade_train_backward(frame, ws, x, T, view, view_orig, rotate_normal, ray_augm, g_s, g_rgb, kept=None):
    """Recomputes the forward and returns the per-sample gradient dL/dx (P,3), the FiLM gradients (6,256) x 2 and the
    operand streams of the weight-gradient GEMMs (dict of dense (P, width) tensors, see ArahTrainGrads)."""
    lib = load_library()
    x, view, g_s, g_rgb = _f32(x), _f32(view), _f32(g_s), _f32(g_rgb)
    T = _f32(T) if (T is not None and rotate_normal) else None
    vo = _f32(view_orig) if (view_orig is not None and ray_augm) else None
    n, dev = x.shape[0], x.device
    buf = ws.ensure(1, 1)
    kin = KIN_PAD[frame.color_mode]
    E = lambda *shape: torch.empty(*shape, device=dev)
    if kept:
        cc, cinp, c2p = kept["cc"], kept["cin_pad"], kept["c2_pad"]
    else:
        cc, cinp, c2p = _grouped(4, n, 256, dev), _grouped(1, n, kin, dev)[0], _grouped(1, n, 128, dev)[0]
    dd = _grouped(4, n, 256, dev)     # delta_1, delta_4, delta_0, delta_3: the order of their partners in `cc` (c_1, c_4, c_2, c_5)
    d2p = _grouped(1, n, 128, dev)[0]
    st = {"sdf": E(n), "rgb4": E(n, 4), "gx4": E(n, 4), "film_freq": E(6, 256), "film_phase": E(6, 256),
          "cin": cinp[:n], "c": kept["c"] if kept else [cc[0, :n], cc[2, :n], c2p[:n], cc[1, :n], cc[3, :n]],
          "d": [dd[2, :n], dd[0, :n], d2p[:n], dd[3, :n], dd[1, :n], E(n, 4)], "cc": cc, "dd": dd,
          "cin_pad": cinp, "c2_pad": c2p, "d2_pad": d2p}   # the *_pad views: whole buffers, padding rows zero (no remainder product)
    st.update(_sdf_streams(n, dev))
    g = ArahTrainGrads()
    for k in ("sdf", "rgb4", "gx4", "film_freq", "film_phase", "cin"):
        setattr(g, k, _ptr(st[k]))
    for k in ("h", "hd", "av", "avd", "c", "d"):
        arr = getattr(g, k)
        for i, t in enumerate(st[k]):
            arr[i] = _ptr(t).value
    nslab = lib.arah_shade_train_slab_bytes()
    if getattr(ws, "train_slab", None) is None or ws.train_slab.numel() < nslab:
        ws.train_slab = torch.empty(nslab, dtype=torch.uint8, device=dev)
    tin = _train_in(x, T, view, vo, rotate_normal, ray_augm, g_s, g_rgb)
    if kept:
        tin.tap_cin = _ptr(kept["cin"])
        for i, t in enumerate(kept["c"]):
            tin.tap_c[i] = _ptr(t).value
        tin.fwd_rgb4 = _ptr(kept["rgb4"])
    _check(lib.arah_shade_train_backward(C.byref(frame.handle), C.byref(tin), C.byref(g), _ptr(ws.train_slab),
                                         C.c_size_t(ws.train_slab.numel()), _ptr(buf), C.c_size_t(buf.numel()),
                                         _stream()), "arah_shade_train_backward")
    return st


@_guarded
def composite_train_forward(lengths, offsets, sdf, rgb, z, inv_beta, n_steps, render_last_pt):
    """lengths (R,) int32, offsets (R,) int64 into the compacted per-sample arrays sdf (P,) [metres], rgb (P,3), z (P,);
    inv_beta (1,) -> rgb_map (R,3), acc (R,) = clip(sum of weights, 0, 1)."""
    lib = load_library()
    R, dev = int(lengths.shape[0]), sdf.device
    out_rgb, out_acc = torch.empty(R, 3, device=dev), torch.empty(R, device=dev)
    _check(lib.arah_composite_train_forward(C.c_int32(R), C.c_int32(int(n_steps)), C.c_int32(int(bool(render_last_pt))),
                                            _ptr(lengths), _ptr(offsets), _ptr(sdf), _ptr(rgb), _ptr(z), _ptr(inv_beta),
                                            _ptr(out_rgb), _ptr(out_acc), _stream()), "arah_composite_train_forward")
    return out_rgb, out_acc


@_guarded
def composite_train_backward(lengths, offsets, sdf, rgb, z, inv_beta, n_steps, render_last_pt, g_map, g_acc):
    """-> dL/d sdf (P,), dL/d rgb (P,3), dL/d inv_beta (1,)"""
    lib = load_library()
    R, dev = int(lengths.shape[0]), sdf.device
    g_sdf, g_rgb, g_ib = torch.empty_like(sdf), torch.empty_like(rgb), torch.empty(1, device=dev)
    _check(lib.arah_composite_train_backward(C.c_int32(R), C.c_int32(int(n_steps)), C.c_int32(int(bool(render_last_pt))),
                                             _ptr(lengths), _ptr(offsets), _ptr(sdf), _ptr(rgb), _ptr(z), _ptr(inv_beta),
                                             _ptr(_f32(g_map)), _ptr(_f32(g_acc)), _ptr(g_sdf), _ptr(g_rgb), _ptr(g_ib),
                                             _stream()), "arah_composite_train_backward")
    return g_sdf, g_rgb, g_ib


def mesh_query(verts, faces, pts):
    """Closest point of a triangle mesh and containment for every query point (training samplers, zju_mocap.py:461-543).
    verts (V,3) float32, faces (F,3) int32, pts (P,3) float32 or float64 on one GPU ->
    d2 (P,) float64, face (P,) int32, closest (P,3) float64, bary (P,3) float64, inside (P,) bool."""
    lib = load_library()
    dev = _same_device(verts, faces, pts)
    if verts.dtype != torch.float32 or faces.dtype != torch.int32 or pts.dtype not in (torch.float32, torch.float64):
        raise ValueError("verts float32, faces int32, pts float32 / float64 required")
    verts, faces, pts = verts.contiguous(), faces.contiguous(), pts.contiguous()
    P = pts.shape[0]
    d2 = torch.empty(P, dtype=torch.float64, device=dev)
    face = torch.empty(P, dtype=torch.int32, device=dev)
    closest = torch.empty(P, 3, dtype=torch.float64, device=dev)
    bary = torch.empty(P, 3, dtype=torch.float64, device=dev)
    inside = torch.empty(P, dtype=torch.uint8, device=dev)
    with _on_device(dev):
        scratch = torch.empty(lib.arah_mesh_query_scratch_bytes(), dtype=torch.uint8, device=dev)
        _check(lib.arah_mesh_query(_ptr(verts), C.c_int32(verts.shape[0]), _ptr(faces), C.c_int32(faces.shape[0]), _ptr(pts),
                                   C.c_int32(1 if pts.dtype == torch.float64 else 0), C.c_int32(P), _ptr(d2), _ptr(face),
                                   _ptr(closest), _ptr(bary), _ptr(inside), _ptr(scratch), _stream()), "arah_mesh_query")
    return d2, face, closest, bary, inside.bool()


def _soup(tris, what="tris"):
    if not torch.is_tensor(tris) or tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3) or tris.dtype != torch.float32:
        raise ValueError("%s must be an (F, 3, 3) float32 triangle soup" % what)
    if tris.shape[0] < 1:
        raise ValueError("%s holds no triangle" % what)
    return tris.contiguous()


class MeshIndex:
    """The acceleration structure of `mesh_index`: the device buffer and the triangle soup it was built from."""

    def __init__(self, buf, tris):
        self.buf, self.tris = buf, tris

    @property
    def device(self):
        return self.tris.device

    def header(self):
        """Host copy of the structure's figures (a synchronisation; for tests and tools): cells per axis, cell side, number
        of references, triangles on the big list, status."""
        import struct
        raw = bytes(self.buf[:96].cpu().numpy())
        lo_hi_h = struct.unpack("8d", raw[:64])
        n = struct.unpack("7i", raw[64:92])
        return {"lo": lo_hi_h[0:3], "hi": lo_hi_h[3:6], "h": lo_hi_h[6], "n": n[0:3], "n_cells": n[3], "n_refs": n[4],
                "n_big": n[5], "status": n[6]}


def mesh_index(tris):
    """Uniform grid of triangle references over the soup tris (F,3,3) float32 (finite vertices), with a distance transform of
    its occupied cells (arah_mesh_index_build, csrc/meshdist.hpp) -> MeshIndex for `mesh_closest`.  The buffer's size follows
    from F alone; no host synchronisation."""
    require_gpu()
    lib = load_library()
    tris = _soup(tris)
    dev = _same_device(tris)
    F = int(tris.shape[0])
    with _on_device(dev):
        buf = torch.empty(int(lib.arah_mesh_index_bytes(F)), dtype=torch.uint8, device=dev)
        _check(lib.arah_mesh_index_build(_ptr(tris), C.c_int32(F), _ptr(buf), C.c_size_t(buf.numel()), _stream()),
               "arah_mesh_index_build")
    return MeshIndex(buf, tris)


def mesh_closest(index, pts, want_closest=True, want_tested=False):
    """Exact closest triangle of the indexed soup for every point: pts (P,3) float32 -> d2 (P,) float64, face (P,) int32 (the
    lowest index on ties), closest (P,3) float64 or None, tested (P,) int32 (point-triangle tests made) or None.  d2, face and
    closest are bit-equal to `mesh_query` on verts = tris.reshape(-1, 3), faces = arange."""
    lib = load_library()
    if not isinstance(index, MeshIndex):
        raise ValueError("index must come from mesh_index")
    if not torch.is_tensor(pts) or pts.dim() != 2 or pts.shape[1] != 3 or pts.dtype != torch.float32:
        raise ValueError("pts must be (P, 3) float32")
    dev = _same_device(index.buf, index.tris, pts)
    pts = pts.contiguous()
    P = int(pts.shape[0])
    d2 = torch.empty(P, dtype=torch.float64, device=dev)
    face = torch.empty(P, dtype=torch.int32, device=dev)
    closest = torch.empty(P, 3, dtype=torch.float64, device=dev) if want_closest else None
    tested = torch.empty(P, dtype=torch.int32, device=dev) if want_tested else None
    with _on_device(dev):
        _check(lib.arah_mesh_closest(_ptr(index.buf), C.c_size_t(index.buf.numel()), _ptr(index.tris),
                                     C.c_int32(index.tris.shape[0]), _ptr(pts), C.c_int32(P), _ptr(d2), _ptr(face),
                                     _ptr(closest), _ptr(tested), _stream()), "arah_mesh_closest")
    return d2, face, closest, tested


RAY_MODES = {"first": 0, "any": 1}


def mesh_raycast(index, origins, dirs, t_min=0.0, t_max=float("inf"), cull="none", mode="first", want_tested=False, workgroup=None):
    """Rays against the indexed soup (arah_mesh_raycast, csrc/meshray.hpp): index from `mesh_index`, origins and dirs (R,3) float32 on
    its device.  mode="first" -> t (R,) float64, face (R,) int32, bary (R,3) float64, tested (R,) int32 (ray-triangle tests made) or
    None: meshing.mesh_raycast on index.tris bit for bit (a miss: +inf, -1, 0).  mode="any" -> hit (R,) bool, tested: whether any
    face is accepted in [t_min, t_max]; the walk stops at the first.  cull "none" / "back" / "front" as in the specification.  Every
    ray of an index built from a soup with a non-finite vertex misses.  workgroup: 64, 128 or 256 threads instead of the built-in
    size (arah_mesh_raycast_debug; the results are the same for every choice), for measuring it.  No host synchronisation."""
    from . import meshing
    lib = load_library()
    if not isinstance(index, MeshIndex):
        raise ValueError("index must come from mesh_index")
    t_min, t_max, cull_code = meshing.check_raycast_args(index.tris, origins, dirs, t_min, t_max, cull, "mesh_raycast")
    if mode not in RAY_MODES:
        raise ValueError("mesh_raycast: mode must be 'first' or 'any', got %r" % (mode,))
    if workgroup is not None and workgroup not in (64, 128, 256):
        raise ValueError("mesh_raycast: workgroup must be 64, 128 or 256, got %r" % (workgroup,))
    dev = _same_device(index.buf, index.tris, origins, dirs)
    origins, dirs = origins.detach().contiguous(), dirs.detach().contiguous()
    R = int(origins.shape[0])
    first = mode == "first"
    t = torch.empty(R, dtype=torch.float64, device=dev) if first else None
    face = torch.empty(R, dtype=torch.int32, device=dev) if first else None
    bary = torch.empty(R, 3, dtype=torch.float64, device=dev) if first else None
    hit = None if first else torch.empty(R, dtype=torch.uint8, device=dev)
    tested = torch.empty(R, dtype=torch.int32, device=dev) if want_tested else None
    with _on_device(dev):
        head = (_ptr(index.buf), C.c_size_t(index.buf.numel()), _ptr(index.tris), C.c_int32(index.tris.shape[0]), _ptr(origins),
                _ptr(dirs), C.c_int32(R), C.c_double(t_min), C.c_double(t_max), C.c_int32(cull_code), C.c_int32(RAY_MODES[mode]))
        tail = (_ptr(t), _ptr(face), _ptr(bary), _ptr(hit), _ptr(tested), _stream())
        if workgroup is None:
            _check(lib.arah_mesh_raycast(*head, *tail), "arah_mesh_raycast")
        else:
            _check(lib.arah_mesh_raycast_debug(*head, C.c_int32(int(workgroup)), *tail), "arah_mesh_raycast_debug")
    if first:
        return t, face, bary, tested
    return hit.bool(), tested


class ContainsIndex:
    """The acceleration structure of `contains_index`: libmesh's two-dimensional triangle hash on the device (csrc/meshcontains.hpp).
    buf holds the bounds, per-triangle records and the cells' starts, refs the triangle ids of every cell."""

    def __init__(self, buf, refs, n_faces, resolution, n_refs, valid):
        self.buf, self.refs = buf, refs
        self.n_faces, self.resolution, self.n_refs, self.valid = int(n_faces), int(resolution), int(n_refs), bool(valid)

    @property
    def device(self):
        return self.buf.device

    def _head(self):
        return (_ptr(self.buf), C.c_size_t(self.buf.numel()), C.c_int32(self.n_faces), C.c_int32(self.resolution), _ptr(self.refs),
                C.c_int64(self.n_refs))


def _contains_header(buf):
    import struct
    raw = bytes(buf[:88].cpu().numpy())
    n_refs, = struct.unpack("q", raw[56:64])
    n_faces, resolution, valid, status = struct.unpack("4i", raw[64:80])
    return {"scale": struct.unpack("3d", raw[0:24]), "translate": struct.unpack("3d", raw[24:48]), "n_refs": n_refs,
            "n_faces": n_faces, "resolution": resolution, "valid": valid, "status": status,
            "n_med": struct.unpack("I", raw[80:84])[0], "n_huge": struct.unpack("I", raw[84:88])[0]}


def contains_index(verts, faces, resolution=512):
    """libmesh's triangle hash of the mesh verts (V,3) float32, faces (F,3) int32 on one GPU, at `resolution` cells per axis of the xy
    plane (arah_contains_index_count / arah_contains_index_fill) -> ContainsIndex for `mesh_contains` and `mesh_contains_grid`.  The
    number of references depends on the data: it is read back once, which is the index's one host synchronisation.  F = 0 and the
    other degenerate meshes of meshing.mesh_contains give an index against which every point is outside."""
    from . import meshing
    require_gpu()
    lib = load_library()
    res = meshing.check_contains_args(verts, faces, None, resolution, "contains_index")
    if verts.dtype != torch.float32 or faces.dtype != torch.int32:
        raise ValueError("contains_index: verts float32 and faces int32 required")
    dev = _same_device(verts, faces)
    verts, faces = verts.detach().contiguous(), faces.contiguous()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    with _on_device(dev):
        buf = torch.empty(int(lib.arah_contains_index_bytes(F, res)), dtype=torch.uint8, device=dev)
        _check(lib.arah_contains_index_count(_ptr(verts) if F else None, C.c_int32(V), _ptr(faces) if F else None, C.c_int32(F),
                                             C.c_int32(res), _ptr(buf), C.c_size_t(buf.numel()), _stream()), "arah_contains_index_count")
        head = _contains_header(buf)
        n_refs = int(head["n_refs"])
        if n_refs > 2 ** 31 - 1 or head["status"] & 1:
            _check(lib.arah_contains_index_fill(_ptr(buf), C.c_size_t(buf.numel()), C.c_int32(F), C.c_int32(res), None,
                                                C.c_int64(n_refs), _stream()), "arah_contains_index_fill (%d references)" % n_refs)
        refs = torch.empty(n_refs, dtype=torch.int32, device=dev) if n_refs else None
        _check(lib.arah_contains_index_fill(_ptr(buf), C.c_size_t(buf.numel()), C.c_int32(F), C.c_int32(res), _ptr(refs),
                                            C.c_int64(n_refs), _stream()), "arah_contains_index_fill")
    return ContainsIndex(buf, refs, F, res, n_refs, head["valid"])


def mesh_contains(index, pts, want_ambiguous=False, want_tested=False):
    """Which points lie inside the indexed mesh (arah_mesh_contains): pts (P,3) float32 or float64 on the index's device -> inside
    (P,) bool, ambiguous (P,) bool or None, tested (P,) int32 (candidate triangles of the point's cell) or None; equal to
    meshing.mesh_contains bit for bit.  No host synchronisation."""
    lib = load_library()
    if not isinstance(index, ContainsIndex):
        raise ValueError("index must come from contains_index")
    if not torch.is_tensor(pts) or pts.dim() != 2 or pts.shape[1] != 3 or pts.dtype not in (torch.float32, torch.float64):
        raise ValueError("pts must be (P, 3) float32 or float64")
    dev = _same_device(index.buf, index.refs, pts)
    pts = pts.detach().contiguous()
    P = int(pts.shape[0])
    if P > 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 1 points")
    inside = torch.empty(P, dtype=torch.uint8, device=dev)
    ambiguous = torch.empty(P, dtype=torch.uint8, device=dev) if want_ambiguous else None
    tested = torch.empty(P, dtype=torch.int32, device=dev) if want_tested else None
    with _on_device(dev):
        _check(lib.arah_mesh_contains(*index._head(), _ptr(pts) if P else None, C.c_int32(1 if pts.dtype == torch.float64 else 0),
                                      C.c_int32(P), _ptr(inside) if P else None, _ptr(ambiguous) if P else None,
                                      _ptr(tested) if P else None, _stream()), "arah_mesh_contains")
    return inside.bool(), None if ambiguous is None else ambiguous.bool(), tested


def mesh_contains_grid(index, xs, ys, zs):
    """The lattice xs (Nx,) x ys (Ny,) x zs (Nz,) float32 against the indexed mesh (arah_mesh_contains_grid) -> occupancy (Nx,Ny,Nz)
    bool, equal to `mesh_contains` on torch.meshgrid(xs, ys, zs, indexing="ij") bit for bit, and the number of ambiguous lattice
    points, a 0-dim int64 tensor on the device.  The 2-D test runs once per (column, candidate).  No host synchronisation."""
    lib = load_library()
    if not isinstance(index, ContainsIndex):
        raise ValueError("index must come from contains_index")
    for name, x in (("xs", xs), ("ys", ys), ("zs", zs)):
        if not torch.is_tensor(x) or x.dim() != 1 or x.dtype != torch.float32 or x.shape[0] < 1:
            raise ValueError("%s must be a non-empty 1-D float32 tensor" % name)
    dev = _same_device(index.buf, index.refs, xs, ys, zs)
    xs, ys, zs = xs.detach().contiguous(), ys.detach().contiguous(), zs.detach().contiguous()
    nx, ny, nz = int(xs.shape[0]), int(ys.shape[0]), int(zs.shape[0])
    if nx * ny > 2 ** 31 - 1 or nx * ny * nz > 2 ** 33:
        raise ValueError("mesh_contains_grid: at most 2^31 - 1 columns and 2^33 lattice points")
    occ = torch.empty(nx, ny, nz, dtype=torch.uint8, device=dev)
    amb = torch.empty((), dtype=torch.int64, device=dev)
    with _on_device(dev):
        _check(lib.arah_mesh_contains_grid(*index._head(), _ptr(xs), C.c_int32(nx), _ptr(ys), C.c_int32(ny), _ptr(zs), C.c_int32(nz),
                                           _ptr(occ), _ptr(amb), _stream()), "arah_mesh_contains_grid")
    return occ.bool(), amb


class WindingIndex:
    """The cluster tree of `winding_index` on the device (csrc/meshwinding.hpp), the tables of meshing.winding_tree: buf (header and
    build scratch), order (F,) int32, tris (F,3,3) float32 in list order, node_i (N,4) int32 = first, count, level, skip, node_f (N,8)
    float64 = centroid, radius, area vector, area; orient (+1 / -1), volume, n_faces, n_verts, depth, n_nodes, valid (False: a used vertex is
    not finite, every winding number is NaN), lo and side of the cube."""

    def __init__(self, buf, order, tris, node_i, node_f, head, n_verts):
        self.buf, self.order, self.tris, self.node_i, self.node_f = buf, order, tris, node_i, node_f
        self.n_verts = int(n_verts)
        self.n_faces, self.depth, self.n_nodes = int(head["n_faces"]), int(head["depth"]), int(head["n_nodes"])
        self.orient, self.volume, self.valid = int(head["orient"]), float(head["volume"]), bool(head["valid"])
        self.lo, self.side = tuple(head["lo"]), float(head["side"])

    @property
    def device(self):
        return self.buf.device

    def _head(self):
        return (_ptr(self.buf), C.c_size_t(self.buf.numel()), C.c_int32(self.n_faces), C.c_int32(self.depth),
                _ptr(self.tris) if self.n_faces else None, _ptr(self.node_i) if self.n_nodes else None,
                _ptr(self.node_f) if self.n_nodes else None, C.c_int64(self.n_nodes))

    def tree(self):
        """The tables as a meshing.WindingTree on the host (a synchronisation): what meshing.mesh_winding walks."""
        from . import meshing
        ni, nf = self.node_i.cpu(), self.node_f.cpu()
        return meshing.WindingTree(order=self.order.cpu(), tris=self.tris.cpu(), first=ni[:, 0].contiguous(), count=ni[:, 1].contiguous(),
                                   level=ni[:, 2].contiguous(), skip=ni[:, 3].contiguous(), nvec=nf[:, 4:7].contiguous(),
                                   centroid=nf[:, 0:3].contiguous(), radius=nf[:, 3].contiguous(), area=nf[:, 7].contiguous(),
                                   lo=torch.tensor(self.lo, dtype=torch.float64), side=self.side, depth=self.depth,
                                   n_faces=self.n_faces, orient=self.orient, volume=self.volume, valid=self.valid)


def _winding_header(buf):
    import struct
    raw = bytes(buf[:72].cpu().numpy())
    n_faces, depth, valid, status, orient = struct.unpack("5i", raw[48:68])
    return {"lo": struct.unpack("3d", raw[0:24]), "side": struct.unpack("d", raw[24:32])[0], "volume": struct.unpack("d", raw[32:40])[0],
            "n_nodes": struct.unpack("q", raw[40:48])[0], "n_faces": n_faces, "depth": depth, "valid": valid, "status": status,
            "orient": orient}


def winding_index(verts, faces, depth=None):
    """The cluster tree of the fast winding number of the mesh verts (V,3) float32, faces (F,3) int32 on one GPU
    (arah_winding_index_count / arah_winding_index_fill) -> WindingIndex for `mesh_winding` and `mesh_winding_grid`; the tables of
    meshing.winding_tree, the float ones bit for bit.  depth: None for meshing.winding_depth(F), or 0 .. 7.  The number of nodes
    depends on the data: it is read back once, which is the index's one host synchronisation.  A face id outside [0, V) raises, and
    so does a mesh that puts more than meshing.WINDING_MAX_LEAF faces into one leaf cell at depth > 0: the ranking of a cell's faces is
    quadratic in the cell, and the kernel leaves such a cell unranked."""
    from . import meshing
    require_gpu()
    lib = load_library()
    if (not torch.is_tensor(verts) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32
            or not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32):
        raise ValueError("winding_index: verts (V, 3) float32 and faces (F, 3) int32 required")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if F > meshing.WINDING_MAX_FACES:
        raise ValueError("winding_index: at most 2^28 faces")
    depth = meshing.check_winding_depth(depth, F, "winding_index")
    dev = _same_device(verts, faces)
    verts, faces = verts.detach().contiguous(), faces.contiguous()
    if F and V < 1:
        raise ValueError("winding_index: a face names a vertex outside [0, 0)")
    with _on_device(dev):
        buf = torch.empty(int(lib.arah_winding_index_bytes(F, depth)), dtype=torch.uint8, device=dev)
        order = torch.empty(F, dtype=torch.int32, device=dev)
        tris = torch.empty(F, 3, 3, dtype=torch.float32, device=dev)
        _check(lib.arah_winding_index_count(_ptr(verts) if F else None, C.c_int32(V), _ptr(faces) if F else None, C.c_int32(F),
                                            C.c_int32(depth), _ptr(buf), C.c_size_t(buf.numel()), _ptr(order) if F else None,
                                            _ptr(tris) if F else None, _stream()), "arah_winding_index_count")
        head = _winding_header(buf)
        if head["status"] & 1:
            raise ValueError("winding_index: a face names a vertex outside [0, %d)" % V)
        if head["status"] & 2:
            raise ValueError("winding_index: at depth %d one leaf cell holds more than %d of the %d faces (a small fragment far from "
                             "the rest stretches the cube); give another depth, or depth=0 for the brute force"
                             % (depth, meshing.WINDING_MAX_LEAF, F))
        N = int(head["n_nodes"])
        if N > 2 ** 31 - 1:
            _check(lib.arah_winding_index_fill(_ptr(buf), C.c_size_t(buf.numel()), C.c_int32(F), C.c_int32(depth), None, None, None,
                                               C.c_int64(N), _stream()), "arah_winding_index_fill (%d nodes)" % N)
        node_i = torch.empty(N, 4, dtype=torch.int32, device=dev)
        node_f = torch.empty(N, 8, dtype=torch.float64, device=dev)
        _check(lib.arah_winding_index_fill(_ptr(buf), C.c_size_t(buf.numel()), C.c_int32(F), C.c_int32(depth), _ptr(tris) if F else None,
                                           _ptr(node_i) if N else None, _ptr(node_f) if N else None, C.c_int64(N), _stream()),
               "arah_winding_index_fill")
    return WindingIndex(buf, order, tris, node_i, node_f, head, V)


def _winding_outputs(shape, dev, want_counts):
    w = torch.empty(shape, dtype=torch.float64, device=dev)
    inside = torch.empty(shape, dtype=torch.uint8, device=dev)
    n_exact = torch.empty(shape, dtype=torch.int32, device=dev) if want_counts else None
    n_far = torch.empty(shape, dtype=torch.int32, device=dev) if want_counts else None
    return w, inside, n_exact, n_far


def mesh_winding(index, points, accuracy=3.0, want_counts=False):
    """The generalized winding number of points (P,3) float32 against the indexed mesh (arah_mesh_winding) -> w (P,) float64, inside
    (P,) bool = meshing.winding_inside(w, index.orient), n_exact and n_far (P,) int32 or None.  The walk of meshing.mesh_winding:
    the same near / far decisions, bit-equal dipole terms; accuracy = inf is the exact sum.  No host synchronisation."""
    from . import meshing
    lib = load_library()
    if not isinstance(index, WindingIndex):
        raise ValueError("index must come from winding_index")
    acc = meshing.check_accuracy(accuracy, "mesh_winding")
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("mesh_winding: points must be (P, 3) float32")
    dev = _same_device(index.buf, points)
    pts = points.detach().contiguous()
    P = int(pts.shape[0])
    if P > 2 ** 31 - 1:
        raise ValueError("mesh_winding: at most 2^31 - 1 points")
    w, inside, n_exact, n_far = _winding_outputs((P,), dev, want_counts)
    with _on_device(dev):
        _check(lib.arah_mesh_winding(*index._head(), _ptr(pts) if P else None, C.c_int32(P), C.c_double(acc), _ptr(w) if P else None,
                                     _ptr(inside) if P else None, _ptr(n_exact) if P and want_counts else None,
                                     _ptr(n_far) if P and want_counts else None, _stream()), "arah_mesh_winding")
    return w, inside.bool(), n_exact, n_far


def mesh_winding_grid(index, xs, ys, zs, accuracy=3.0, want_counts=False):
    """The lattice xs (Nx,) x ys (Ny,) x zs (Nz,) float32 against the indexed mesh (arah_mesh_winding_grid) -> w (Nx,Ny,Nz) float64,
    occupancy (Nx,Ny,Nz) bool, n_exact, n_far (Nx,Ny,Nz) int32 or None; equal to `mesh_winding` on torch.meshgrid(xs, ys, zs,
    indexing="ij") bit for bit.  The lattice point is made in the kernel.  No host synchronisation."""
    from . import meshing
    lib = load_library()
    if not isinstance(index, WindingIndex):
        raise ValueError("index must come from winding_index")
    acc = meshing.check_accuracy(accuracy, "mesh_winding_grid")
    for name, x in (("xs", xs), ("ys", ys), ("zs", zs)):
        if not torch.is_tensor(x) or x.dim() != 1 or x.dtype != torch.float32 or x.shape[0] < 1:
            raise ValueError("mesh_winding_grid: %s must be a non-empty 1-D float32 tensor" % name)
    dev = _same_device(index.buf, xs, ys, zs)
    xs, ys, zs = xs.detach().contiguous(), ys.detach().contiguous(), zs.detach().contiguous()
    nx, ny, nz = int(xs.shape[0]), int(ys.shape[0]), int(zs.shape[0])
    if nx * ny * nz > 2 ** 31 - 1:
        raise ValueError("mesh_winding_grid: at most 2^31 - 1 lattice points")
    w, occ, n_exact, n_far = _winding_outputs((nx, ny, nz), dev, want_counts)
    with _on_device(dev):
        _check(lib.arah_mesh_winding_grid(*index._head(), _ptr(xs), C.c_int32(nx), _ptr(ys), C.c_int32(ny), _ptr(zs), C.c_int32(nz),
                                          C.c_double(acc), _ptr(w), _ptr(occ), _ptr(n_exact), _ptr(n_far), _stream()),
               "arah_mesh_winding_grid")
    return w, occ.bool(), n_exact, n_far


SDF_GRID_INFO = ("band", "status", "tests", "lane", "wave", "group", "huge")


def read_sdf_grid_info(info):
    """Host copy of arah_mesh_sdf_grid's counters (a synchronisation): nodes in the band, status, point-triangle tests made and the
    triangles of the four size classes."""
    v = [int(x) for x in info.cpu().tolist()]
    tests = (v[2] & 0xffffffff) | ((v[3] & 0xffffffff) << 32)
    return dict(zip(SDF_GRID_INFO, (v[0], v[1], tests, v[4], v[5], v[6], v[7])))


def mesh_sdf_grid(tris, xs, ys, zs, trunc, occupancy=None, want_face=False, want_info=False):
    """The truncated distance field of the soup tris (F,3,3) float32 (F may be 0) on the lattice xs (Nx,) x ys (Ny,) x zs (Nz,)
    float32, each strictly ascending (arah_mesh_sdf_grid, csrc/meshsdf.hpp) -> d2 (Nx,Ny,Nz) float64 (+inf outside the band of width
    trunc), face (Nx,Ny,Nz) int32 or None, sdf (Nx,Ny,Nz) float32 by meshing.signed_distance from `occupancy` (bool or uint8, as
    `mesh_contains_grid` returns it; None: every node outside, the unsigned distance), info (8,) int32 on the device or None (see
    `read_sdf_grid_info`).  d2 and face equal meshing.mesh_sdf_grid bit for bit.  The axes' order is the caller's to guarantee
    (geometry.mesh_sdf_grid checks it).  No host synchronisation."""
    from . import meshing
    require_gpu()
    lib = load_library()
    if not torch.is_tensor(tris) or tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3) or tris.dtype != torch.float32:
        raise ValueError("mesh_sdf_grid: tris must be an (F, 3, 3) float32 triangle soup")
    trunc = meshing.check_trunc(trunc, "mesh_sdf_grid")
    for name, x in (("xs", xs), ("ys", ys), ("zs", zs)):
        if not torch.is_tensor(x) or x.dim() != 1 or x.dtype != torch.float32 or x.shape[0] < 1:
            raise ValueError("mesh_sdf_grid: %s must be a non-empty 1-D float32 tensor" % name)
    nx, ny, nz = int(xs.shape[0]), int(ys.shape[0]), int(zs.shape[0])
    if nx * ny * nz > 2 ** 31 - 1:
        raise ValueError("mesh_sdf_grid: at most 2^31 - 1 lattice nodes, got %d x %d x %d" % (nx, ny, nz))
    if occupancy is not None:
        if (not torch.is_tensor(occupancy) or tuple(occupancy.shape) != (nx, ny, nz)
                or occupancy.dtype not in (torch.bool, torch.uint8)):
            raise ValueError("mesh_sdf_grid: occupancy must be a (%d, %d, %d) bool or uint8 tensor" % (nx, ny, nz))
        occupancy = occupancy.contiguous().view(torch.uint8)
    dev = _same_device(tris, xs, ys, zs, occupancy)
    tris = tris.detach().contiguous()
    xs, ys, zs = xs.detach().contiguous(), ys.detach().contiguous(), zs.detach().contiguous()
    F = int(tris.shape[0])
    d2 = torch.empty(nx, ny, nz, dtype=torch.float64, device=dev)
    face = torch.empty(nx, ny, nz, dtype=torch.int32, device=dev) if want_face else None
    sdf = torch.empty(nx, ny, nz, dtype=torch.float32, device=dev)
    info = torch.empty(8, dtype=torch.int32, device=dev)
    with _on_device(dev):
        nbytes = int(lib.arah_mesh_sdf_grid_bytes(F, nx, ny, nz))
        if nbytes == 0:
            raise ValueError("mesh_sdf_grid: %d faces on %d x %d x %d nodes is out of range" % (F, nx, ny, nz))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _check(lib.arah_mesh_sdf_grid(_ptr(tris) if F else None, C.c_int32(F), _ptr(xs), C.c_int32(nx), _ptr(ys), C.c_int32(ny),
                                      _ptr(zs), C.c_int32(nz), C.c_float(trunc), _ptr(occupancy), _ptr(d2), _ptr(face), _ptr(sdf),
                                      _ptr(info), _ptr(scratch), C.c_size_t(nbytes), _stream()), "arah_mesh_sdf_grid")
    return d2, face, sdf, info if want_info else None


def face_area_cumsum(tris):
    """Running sum of the areas of the soup's triangles, (F,) float64 on the device (arah_face_area_cumsum): float64 cross
    products, one fixed summation order -- bit-reproducible, unlike torch.cumsum on the device for arrays of this size."""
    lib = load_library()
    tris = _soup(tris)
    dev = _same_device(tris)
    with _on_device(dev):
        cum = torch.empty(tris.shape[0], dtype=torch.float64, device=dev)
        _check(lib.arah_face_area_cumsum(_ptr(tris), C.c_int32(tris.shape[0]), _ptr(cum), _stream()), "arah_face_area_cumsum")
    return cum


SURFACE_METRICS = ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "normal_consistency", "hausdorff_ab", "hausdorff_ba",
                   "n_a", "n_b")


def surface_metrics(tris_a, sample_face_a, d2_ab, face_ab, tris_b, sample_face_b, d2_ba, face_ba):
    """The geometry scores (arah_surface_metrics) from the samples' faces and their query results against the other mesh ->
    (9,) float64 on the device in the order of SURFACE_METRICS.  No atomics, fixed summation order, no host synchronisation."""
    lib = load_library()
    tris_a, tris_b = _soup(tris_a, "tris_a"), _soup(tris_b, "tris_b")
    dev = _same_device(tris_a, sample_face_a, d2_ab, face_ab, tris_b, sample_face_b, d2_ba, face_ba)
    n_a, n_b = int(d2_ab.shape[0]), int(d2_ba.shape[0])
    if n_a < 1 or n_b < 1:
        raise ValueError("at least one sample per mesh required")
    for t, n, dt in ((sample_face_a, n_a, torch.int32), (face_ab, n_a, torch.int32), (d2_ab, n_a, torch.float64),
                     (sample_face_b, n_b, torch.int32), (face_ba, n_b, torch.int32), (d2_ba, n_b, torch.float64)):
        if t.dtype != dt or tuple(t.shape) != (n,):
            raise ValueError("faces int32 (n,), d2 float64 (n,) required")
    args = [t.contiguous() for t in (sample_face_a, d2_ab, face_ab, sample_face_b, d2_ba, face_ba)]
    with _on_device(dev):
        out = torch.empty(len(SURFACE_METRICS), dtype=torch.float64, device=dev)
        scratch = torch.empty(int(lib.arah_surface_metrics_bytes(n_a, n_b)), dtype=torch.uint8, device=dev)
        _check(lib.arah_surface_metrics(_ptr(tris_a), C.c_int32(tris_a.shape[0]), _ptr(args[0]), _ptr(args[1]), _ptr(args[2]),
                                        C.c_int32(n_a), _ptr(tris_b), C.c_int32(tris_b.shape[0]), _ptr(args[3]), _ptr(args[4]),
                                        _ptr(args[5]), C.c_int32(n_b), _ptr(out), _ptr(scratch), C.c_size_t(scratch.numel()),
                                        _stream()), "arah_surface_metrics")
    return out


def _cloud(points, what="points"):
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("%s must be (P, 3) float32" % what)
    if points.shape[0] < 1:
        raise ValueError("%s holds no point" % what)
    return points.contiguous()


class PointIndex:
    """The acceleration structure of `point_index`: the device buffer and the cloud it was built from."""
    # the layout of csrc/pointdist.hpp: PdHeader (11 doubles, then n[3], n_cells, n_refs, n_bad, cn[3], c_occ, c_occ2) and the
    # blocks carve_point_index() hands out before cell_base, each rounded up to 256 bytes
    _HEADER = "11d11i"
    _N_BAD = 11 * 8 + 5 * 4                 # byte offset of PdHeader.n_bad
    _HEADER_BYTES, _STAT_BLOCKS, _COARSE = 256, 256, 64       # kPdHeaderBytes, kPdStatBlocks, kPdCoarse

    @classmethod
    def _cell_base_offset(cls):
        up = lambda b: (b + 255) // 256 * 256
        return up(cls._HEADER_BYTES) + up(8 * 8 * cls._STAT_BLOCKS) + up(4 * (cls._COARSE + 1) ** 3)

    def __init__(self, buf, points):
        self.buf, self.points = buf, points

    @property
    def device(self):
        return self.points.device

    @property
    def n_bad(self):
        """0-dim int32 DEVICE tensor: the cloud's points with a non-finite coordinate (skipped by the index).  No
        synchronisation."""
        return self.buf[self._N_BAD:self._N_BAD + 4].view(torch.int32)[0]

    def header(self):
        """Host copy of the structure's figures (a synchronisation; for tests and tools): box, cell side h, coarse cell side g,
        measured dimension, cells per axis n, n_cells, n_refs (finite points), n_bad, the coarse lattice cn and its occupied
        cells c_occ / occupied 2x2x2 blocks c_occ2."""
        import struct
        d = struct.unpack(self._HEADER, bytes(self.buf[:struct.calcsize(self._HEADER)].cpu().numpy()))
        return {"lo": d[0:3], "hi": d[3:6], "h": d[6], "g": d[8], "dim": d[10], "n": d[11:14], "n_cells": d[14], "n_refs": d[15],
                "n_bad": d[16], "cn": d[17:20], "c_occ": d[20], "c_occ2": d[21]}

    def cell_counts(self):
        """Points per cell, (n_cells,) int32 on the device (a synchronisation: the header is read; for tests and tools)."""
        n_cells = self.header()["n_cells"]
        off = self._cell_base_offset()
        base = self.buf[off:off + 4 * (n_cells + 1)].view(torch.int32)
        return base[1:] - base[:-1]


def point_index(points):
    """Uniform grid over the cloud points (P,3) float32 with a distance transform of its occupied cells
    (arah_point_index_build, csrc/pointdist.hpp) -> PointIndex for `point_nearest`.  Points with a non-finite coordinate are
    skipped.  The buffer's size follows from P alone; no host synchronisation."""
    points = _cloud(points)
    require_gpu()
    lib = load_library()
    dev = _same_device(points)
    P = int(points.shape[0])
    with _on_device(dev):
        buf = torch.empty(int(lib.arah_point_index_bytes(P)), dtype=torch.uint8, device=dev)
        _check(lib.arah_point_index_build(_ptr(points), C.c_int32(P), _ptr(buf), C.c_size_t(buf.numel()), _stream()),
               "arah_point_index_build")
    return PointIndex(buf, points)


def point_nearest(index, pts, want_tested=False):
    """Exact nearest point of the indexed cloud for every query: pts (Q,3) float32 -> d2 (Q,) float64, nearest (Q,) int32 (the
    lowest index on ties), tested (Q,) int32 (point tests made) or None.  A non-finite query answers (NaN, -1), a cloud without
    a finite point (+inf, -1)."""
    if not isinstance(index, PointIndex):
        raise ValueError("index must come from point_index")
    if not torch.is_tensor(pts) or pts.dim() != 2 or pts.shape[1] != 3 or pts.dtype != torch.float32:
        raise ValueError("pts must be (Q, 3) float32")
    lib = load_library()
    dev = _same_device(index.buf, index.points, pts)
    pts = pts.contiguous()
    Q = int(pts.shape[0])
    d2 = torch.empty(Q, dtype=torch.float64, device=dev)
    nearest = torch.empty(Q, dtype=torch.int32, device=dev)
    tested = torch.empty(Q, dtype=torch.int32, device=dev) if want_tested else None
    with _on_device(dev):
        _check(lib.arah_point_nearest(_ptr(index.buf), C.c_size_t(index.buf.numel()), _ptr(index.points),
                                      C.c_int32(index.points.shape[0]), _ptr(pts), C.c_int32(Q), _ptr(d2), _ptr(nearest),
                                      _ptr(tested), _stream()), "arah_point_nearest")
    return d2, nearest, tested


MAX_THRESHOLDS = 16
SAMPLE_SUMS = ("sum_d", "sum_d2", "sum_c", "max_d", "n", "n_c")


def sample_scores(d2, sample_normals=None, other_normals=None, idx=None, thr2=None):
    """One side of the geometry scores (arah_sample_scores): d2 (n,) float64 of its samples; optionally the samples' unit
    normals (n,3) float64 with the other side's unit normals (m,3) float64 and idx (n,) int32 into them; thr2 (T,) float64
    DEVICE tensor of squared thresholds, T <= 16, or None -> (sums (6,) float64 in the order of SAMPLE_SUMS, within (T,) int64:
    the samples with d2 <= thr2[t]), both on the device.  Fixed summation order, no floating-point atomics, no host
    synchronisation."""
    if not torch.is_tensor(d2) or d2.dim() != 1 or d2.dtype != torch.float64 or d2.shape[0] < 1:
        raise ValueError("d2 must be (n,) float64 with n >= 1")
    n = int(d2.shape[0])
    normals = sample_normals is not None or other_normals is not None
    if normals:
        if sample_normals is None or other_normals is None or idx is None:
            raise ValueError("sample_normals, other_normals and idx come together")
        for t, shape in ((sample_normals, (n, 3)), (other_normals, None)):
            if not torch.is_tensor(t) or t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1 \
                    or (shape is not None and tuple(t.shape) != shape):
                raise ValueError("normals must be (n, 3) / (m, 3) float64")
        if not torch.is_tensor(idx) or idx.dtype != torch.int32 or tuple(idx.shape) != (n,):
            raise ValueError("idx must be (n,) int32")
    T = 0
    if thr2 is not None:
        if not torch.is_tensor(thr2) or thr2.dtype != torch.float64 or thr2.dim() != 1 or not 1 <= thr2.shape[0] <= MAX_THRESHOLDS:
            raise ValueError("thr2 must be (T,) float64 with 1 <= T <= %d" % MAX_THRESHOLDS)
        T = int(thr2.shape[0])
    lib = load_library()
    dev = _same_device(d2, sample_normals, other_normals, idx, thr2)
    d2 = d2.contiguous()
    if normals:
        sample_normals, other_normals, idx = sample_normals.contiguous(), other_normals.contiguous(), idx.contiguous()
    thr2 = thr2.contiguous() if T else None
    with _on_device(dev):
        sums = torch.empty(len(SAMPLE_SUMS), dtype=torch.float64, device=dev)
        within = torch.empty(T, dtype=torch.int64, device=dev)
        scratch = torch.empty(int(lib.arah_sample_scores_bytes(n)), dtype=torch.uint8, device=dev)
        _check(lib.arah_sample_scores(_ptr(d2), C.c_int32(n), _ptr(sample_normals), _ptr(other_normals),
                                      C.c_int32(other_normals.shape[0] if normals else 0), _ptr(idx), _ptr(thr2), C.c_int32(T),
                                      _ptr(sums), _ptr(within) if T else None, _ptr(scratch), C.c_size_t(scratch.numel()), _stream()),
               "arah_sample_scores")
    return sums, within


def gram_skinny(a, b):
    """a^T b for a (P, m <= 4) and b (P, n), row strides free (column slices of wider streams are fine): (m, n)."""
    lib = load_library()
    dev = _same_device(a, b)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.stride(1) != 1 or b.stride(1) != 1:
        raise ValueError("float32 operands with unit column stride required")
    P, m = a.shape
    n = b.shape[1]
    if P == 0:
        return torch.zeros(m, n, device=dev)
    with _on_device(dev):
        blocks = lib.arah_gram_skinny_blocks(C.c_int32(P))
        partial = torch.empty(blocks, m, n, device=dev)
        _check(lib.arah_gram_skinny(C.c_void_p(a.data_ptr()), C.c_int32(a.stride(0)), C.c_int32(m),
                                    C.c_void_p(b.data_ptr()), C.c_int32(b.stride(0)),
                                    C.c_int32(n), C.c_int32(P), _ptr(partial), _stream()), "arah_gram_skinny")
    return partial.sum(0)


def colsum(a, scale=None):
    """y[c] = sum_r scale[r] a[r, c] for a (R, n) fp32 with unit column stride (row stride free), scale (R,) or None: (n,).
    One pass at HBM speed with a fixed summation order (arah_colsum)."""
    lib = load_library()
    dev = _same_device(a, scale)
    if a.dtype != torch.float32 or a.dim() != 2 or a.stride(1) != 1:
        raise ValueError("colsum: (R, n) float32 with unit column stride required")
    R, n = a.shape
    sc = None if scale is None else _f32(scale).reshape(-1)
    if sc is not None and sc.numel() != R:
        raise ValueError("colsum: one scale per row")
    with _on_device(dev):
        y = torch.empty(n, device=dev)
        partial = torch.empty(max(1, int(lib.arah_colsum_blocks(C.c_int64(R)))), n, device=dev)
        _check(lib.arah_colsum(C.c_void_p(a.data_ptr()), C.c_int64(a.stride(0) if R > 1 else n), C.c_int32(n), C.c_int64(R),
                               _ptr(sc), _ptr(partial), _ptr(y), _stream()), "arah_colsum")
    return y


def hsoftmax_train_forward(logits, scale):
    """(n, 25) raw logits -> (n, 24) weights = hierarchical_softmax(scale * logits) (arah_hsoftmax_train_forward); no autograd."""
    lib = load_library()
    x = _f32(logits)
    dev = _same_device(x)
    with _on_device(dev):
        w = torch.empty(x.shape[0], 24, device=dev)
        _check(lib.arah_hsoftmax_train_forward(_ptr(x), C.c_int32(x.shape[0]), C.c_float(float(scale)), _ptr(w), _stream()),
               "arah_hsoftmax_train_forward")
    return w


def hsoftmax_train_backward(logits, scale, g_w):
    """d L / d logits (n, 25) for upstream gradients g_w (n, 24) on hierarchical_softmax(scale * logits)."""
    lib = load_library()
    x, g = _f32(logits), _f32(g_w)
    dev = _same_device(x, g)
    with _on_device(dev):
        gx = torch.empty_like(x)
        _check(lib.arah_hsoftmax_train_backward(_ptr(x), C.c_int32(x.shape[0]), C.c_float(float(scale)), _ptr(g), _ptr(gx),
                                                _stream()), "arah_hsoftmax_train_backward")
    return gx


def _parents_array(parents):
    arr = (C.c_int32 * len(parents))(*[int(p) for p in parents])
    return arr


def pose_tree_forward(own, glob, W1, b1, W2, b2, parents):
    """own (J,13), glob (6,), stacked per-joint parameters W1 (J,19,19), b1 (J,19), W2 (J,6,19), b2 (J,6), parents (list, -1 = root)
    -> feats (J,6), hidden (J,19) (arah_pose_tree_forward); no autograd."""
    lib = load_library()
    ts = [_f32(t) for t in (own, glob, W1, b1, W2, b2)]
    dev = _same_device(*ts)
    J = ts[0].shape[0]
    if ts[0].shape != (J, 13) or ts[1].numel() != 6 or ts[2].shape != (J, 19, 19) or ts[3].shape != (J, 19) \
            or ts[4].shape != (J, 6, 19) or ts[5].shape != (J, 6) or len(parents) != J:
        raise ValueError("pose_tree_forward: shapes of a 13 + 6 -> 19 -> 6 tree encoder expected")
    with _on_device(dev):
        feats, hidden = torch.empty(J, 6, device=dev), torch.empty(J, 19, device=dev)
        _check(lib.arah_pose_tree_forward(*[_ptr(t) for t in ts], _parents_array(parents), C.c_int32(J), _ptr(feats), _ptr(hidden),
                                          _stream()), "arah_pose_tree_forward")
    return feats, hidden


def pose_tree_backward(own, glob, W1, W2, parents, feats, hidden, g_feats):
    """-> (gW1, gb1, gW2, gb2, g_glob) for upstream gradients g_feats (J,6) (arah_pose_tree_backward)."""
    lib = load_library()
    own, glob, W1, W2, feats, hidden, g = [_f32(t) for t in (own, glob, W1, W2, feats, hidden, g_feats)]
    dev = _same_device(own, glob, W1, W2, feats, hidden, g)
    J = own.shape[0]
    with _on_device(dev):
        gW1, gb1 = torch.empty(J, 19, 19, device=dev), torch.empty(J, 19, device=dev)
        gW2, gb2, gg = torch.empty(J, 6, 19, device=dev), torch.empty(J, 6, device=dev), torch.empty(6, device=dev)
        _check(lib.arah_pose_tree_backward(_ptr(own), _ptr(glob), _ptr(W1), _ptr(W2), _parents_array(parents), C.c_int32(J),
                                           _ptr(feats), _ptr(hidden), _ptr(g), _ptr(gW1), _ptr(gb1), _ptr(gW2), _ptr(gb2), _ptr(gg),
                                           _stream()), "arah_pose_tree_backward")
    return gW1, gb1, gW2, gb2, gg


def inverse3x3(m, scale=1.0):
    """(scale * m)^-1 for m (P, 3, 3) fp32 by cofactors (arah_inverse3x3); no autograd."""
    lib = load_library()
    mm = _f32(m)
    dev = _same_device(mm)
    if mm.dim() != 3 or mm.shape[1:] != (3, 3):
        raise ValueError("inverse3x3: (P, 3, 3) required")
    with _on_device(dev):
        out = torch.empty_like(mm)
        _check(lib.arah_inverse3x3(_ptr(mm), C.c_int32(mm.shape[0]), C.c_float(float(scale)), _ptr(out), _stream()),
               "arah_inverse3x3")
    return out


@_guarded
def render(frame, ws, sampling, cam_loc, dirs, near_far, pose34, tiered=False, maps=False):
    """Whole eval forward. pose34: DEVICE (3,4) world->camera (no host copy, no stream drain).
    tiered: build the frame's occupancy bitmap first and let arah_render skip the samples it certifies (csrc/tier.hpp;
    lazy shading only -- with full_shading the flag is ignored).
    maps: arah_render_maps -- also the composited normal (world frame, not renormalised) and depth maps (include/arah_hip.h).
    Returns rgb, points_cam, vol_mask, acc, dists, conv (+ normal_world (N,3), depth (N,) with maps)."""
    lib = load_library()
    cam, d, nf = _f32(cam_loc), _f32(dirs), _f32(near_far)
    n, S = d.shape[0], sampling.n_steps
    buf = ws.ensure(n, S)
    cfg = sampling.handle
    if tiered and cfg.full_shading != SHADING_FULL:
        occ = ws.occupancy(frame)
        buf = ws.buf
        cfg = ArahSampling.from_buffer_copy(sampling.handle)   # the bitmap is this frame's: a private copy of the call's struct
        cfg.occupancy = occ.data_ptr()
    dev = d.device
    rgb = torch.empty(n, 3, device=dev)
    pcam = torch.empty(n, 3, device=dev)
    vol = torch.empty(n, dtype=torch.uint8, device=dev)
    acc = torch.empty(n, device=dev)
    dists = torch.empty(n, device=dev)
    conv = torch.empty(n, dtype=torch.uint8, device=dev)
    d_pose = _f32(pose34).reshape(-1)[:12].contiguous()
    if not maps:
        _check(lib.arah_render(C.byref(frame.handle), C.byref(cfg), _ptr(cam), C.c_int32(n // cam.shape[0]),
                               _ptr(d), _ptr(nf), _ptr(d_pose), C.c_int32(n), _ptr(rgb), _ptr(pcam), _ptr(vol), _ptr(acc),
                               _ptr(dists), _ptr(conv), _ptr(buf), C.c_size_t(buf.numel()), _stream()), "arah_render")
        return rgb, pcam, vol, acc, dists, conv
    mbuf = ws.maps_ensure(n, S)
    normal = torch.empty(n, 3, device=dev)
    depth = torch.empty(n, device=dev)
    _check(lib.arah_render_maps(C.byref(frame.handle), C.byref(cfg), _ptr(cam), C.c_int32(n // cam.shape[0]),
                                _ptr(d), _ptr(nf), _ptr(d_pose), C.c_int32(n), _ptr(rgb), _ptr(pcam), _ptr(vol), _ptr(acc),
                                _ptr(dists), _ptr(conv), _ptr(normal), _ptr(depth), _ptr(buf), C.c_size_t(buf.numel()),
                                _ptr(mbuf), C.c_size_t(mbuf.numel()), _stream()), "arah_render_maps")
    return rgb, pcam, vol, acc, dists, conv, normal, depth


@_guarded
def tier_audit(frame, ws, sampling, cam_loc, dirs, near_far, rate_log2=0, seed=0):
    """Audit of the certificate behind the last TIERED render(frame, ws, sampling, ...) of these rays (arah_tier_audit): enqueued on
    the current stream, no synchronisation.  Returns the result block, a device uint8 tensor of AUDIT_BYTES (a view into the
    scratch's audit buffer: the next audit overwrites it) -- audit_result() reads it."""
    lib = load_library()
    cam, d, nf = _f32(cam_loc), _f32(dirs), _f32(near_far)
    n, S = d.shape[0], sampling.n_steps
    if ws.buf is None or ws.occ is None:
        raise RuntimeError("tier_audit: no tiered render on this scratch")
    abuf = ws.audit_ensure(n, S)
    cfg = ArahSampling.from_buffer_copy(sampling.handle)
    cfg.occupancy = ws.occ.data_ptr()
    _check(lib.arah_tier_audit(C.byref(frame.handle), C.byref(cfg), _ptr(cam), C.c_int32(n // cam.shape[0]), _ptr(d), _ptr(nf),
                               C.c_int32(n), C.c_int32(int(rate_log2)), C.c_uint32(int(seed) & 0xffffffff), _ptr(abuf),
                               C.c_size_t(abuf.numel()), _ptr(ws.buf), C.c_size_t(ws.buf.numel()), _stream()), "arah_tier_audit")
    return abuf[:AUDIT_BYTES]


def audit_result(block):
    """ArahTierAudit as a dict, from the result block (a device or host uint8 tensor of AUDIT_BYTES; a device one synchronises)."""
    raw = bytes(block.cpu().numpy().tobytes()) if isinstance(block, torch.Tensor) else bytes(block)
    r = ArahTierAudit.from_buffer_copy(raw[:AUDIT_BYTES])
    k = int(r.n_first)
    out = {name: int(getattr(r, name)) for name, _ in ArahTierAudit._fields_
           if name not in ("first_index", "first_class", "min_ratio", "reserved")}
    out["min_ratio"] = float(r.min_ratio)
    out["first"] = [("ABC"[int(r.first_class[i])], int(r.first_index[i])) for i in range(k)]
    out["violations"] = out["a_violations"] + out["b_violations"] + out["c_violations"]
    return out

