"""Python (ctypes) host harness over the C ABI of libgsplat_hip.so.

This is plumbing for the tests and bench.py: it mirrors the reference's
interface for the hot path -- `Scene.setData`, `Camera.update`,
`renderer.render(scene, camera)` (src/core/Scene.ts:58-180,
src/cameras/Camera.ts:81-92, src/renderers/WebGLRenderer.ts:241-296) -- and
calls the HIP library for everything the GPU does.  There is no CPU fallback:
if the library or a GPU is missing, construction raises.
The Node/JavaScript host (the reference's own language) lives in ../../js.
"""
import ctypes
import os

import numpy as np

from .camera import Camera, orbit_camera, orbit_pose  # noqa: F401
from . import synth  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libgsplat_hip.so"))

GSR_FLAG_TIMING = 1
GSR_FLAG_THROUGHPUT = 2
GSR_ERR_OVERFLOW = -5
GSR_ERR_BUSY = -7


class GsrOptions(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("early_out_eps", ctypes.c_float), ("band_x0", ctypes.c_int32), ("band_x1", ctypes.c_int32),
                ("flags", ctypes.c_int32)]


class GsrTimings(ctypes.Structure):
    _fields_ = [("ms_project_key", ctypes.c_float), ("ms_sort", ctypes.c_float), ("ms_bin", ctypes.c_float),
                ("ms_blend", ctypes.c_float), ("ms_combine", ctypes.c_float), ("ms_total", ctypes.c_float), ("visible", ctypes.c_uint64),
                ("bin_entries", ctypes.c_uint64), ("tile_entries", ctypes.c_uint64), ("n", ctypes.c_uint32), ("frames", ctypes.c_uint32),
                ("sum_ms_project_key", ctypes.c_double), ("sum_ms_sort", ctypes.c_double),
                ("sum_ms_bin", ctypes.c_double), ("sum_ms_blend", ctypes.c_double), ("sum_ms_combine", ctypes.c_double),
                ("sum_ms_total", ctypes.c_double),
                ("sum_visible", ctypes.c_uint64), ("sum_bin_entries", ctypes.c_uint64),
                ("sum_tile_entries", ctypes.c_uint64), ("sum_frames", ctypes.c_uint64),
                ("overflow_frames", ctypes.c_uint64), ("dropped_frames", ctypes.c_uint64)]


class GsrFrame(ctypes.Structure):
    _fields_ = [("pixels", ctypes.c_void_p), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("slot", ctypes.c_int32),
                ("serial", ctypes.c_uint64)]


class GsrDeliveryOptions(ctypes.Structure):
    _fields_ = [("slots", ctypes.c_int32), ("format", ctypes.c_int32), ("full_range", ctypes.c_int32), ("background", ctypes.c_uint8 * 4)]


class GsrFrameLayout(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("planes", ctypes.c_int32),
                ("offset", ctypes.c_uint64 * 3), ("stride", ctypes.c_int32 * 3), ("rows", ctypes.c_int32 * 3), ("bytes", ctypes.c_uint64)]


class GsrDepthDeliveryOptions(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int32), ("step", ctypes.c_int32), ("near", ctypes.c_float), ("reserved", ctypes.c_int32)]


class GsrRegion(ctypes.Structure):
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("x1", ctypes.c_int32), ("y1", ctypes.c_int32), ("mask", ctypes.c_void_p),
                ("mask_stride", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class GsrSelectionBounds(ctypes.Structure):
    _fields_ = [("count", ctypes.c_uint32), ("min", ctypes.c_float * 3), ("max", ctypes.c_float * 3)]


class GsrOverlayOptions(ctypes.Structure):
    _fields_ = [("tint", ctypes.c_float * 3), ("mix", ctypes.c_float), ("reserved", ctypes.c_int32 * 4)]


class GsrOutlineOptions(ctypes.Structure):
    _fields_ = [("rgb", ctypes.c_float * 3), ("alpha", ctypes.c_float), ("threshold", ctypes.c_float), ("width", ctypes.c_int32),
                ("side", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


class GsrNeighbourInfo(ctypes.Structure):
    _fields_ = [("in_scope", ctypes.c_uint32), ("nonfinite", ctypes.c_uint32), ("pair_bound", ctypes.c_uint64), ("budget", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class GsrClusterInfo(ctypes.Structure):
    _fields_ = [("in_scope", ctypes.c_uint32), ("nonfinite", ctypes.c_uint32), ("pair_bound", ctypes.c_uint64), ("budget", ctypes.c_uint64),
                ("core", ctypes.c_uint32), ("border", ctypes.c_uint32), ("noise", ctypes.c_uint32), ("clusters", ctypes.c_uint32),
                ("largest_label", ctypes.c_uint32), ("largest_size", ctypes.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class GsrKnnInfo(ctypes.Structure):
    _fields_ = [("in_scope", ctypes.c_uint32), ("nonfinite", ctypes.c_uint32), ("pair_bound", ctypes.c_uint64), ("budget", ctypes.c_uint64),
                ("complete", ctypes.c_uint32), ("finite_values", ctypes.c_uint32), ("value_min", ctypes.c_double), ("value_max", ctypes.c_double)]

    def as_dict(self):
        return {k: (float if t is ctypes.c_double else int)(getattr(self, k)) for k, t in self._fields_}


class GsrNormalOptions(ctypes.Structure):
    _fields_ = [("source", ctypes.c_int32), ("k", ctypes.c_uint32), ("radius", ctypes.c_double), ("scope", ctypes.c_uint32), ("oriented", ctypes.c_uint32),
                ("budget", ctypes.c_uint64), ("toward", ctypes.c_double * 3)]


class GsrNormalInfo(ctypes.Structure):
    _fields_ = [("in_scope", ctypes.c_uint32), ("nonfinite", ctypes.c_uint32), ("pair_bound", ctypes.c_uint64), ("budget", ctypes.c_uint64),
                ("valid", ctypes.c_uint32), ("variation_min", ctypes.c_double), ("variation_max", ctypes.c_double)]

    def as_dict(self):
        return {k: (float if t is ctypes.c_double else int)(getattr(self, k)) for k, t in self._fields_}


class GsrCellInfo(ctypes.Structure):
    _fields_ = [("in_scope", ctypes.c_uint32), ("candidates", ctypes.c_uint32), ("cells", ctypes.c_uint32), ("merged_cells", ctypes.c_uint32),
                ("merged_members", ctypes.c_uint32), ("largest", ctypes.c_uint32), ("rows_after", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                ("pair_bound", ctypes.c_uint64), ("budget", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


class GsrPlaneInfo(ctypes.Structure):
    _fields_ = [("in_scope", ctypes.c_uint32), ("nonfinite", ctypes.c_uint32), ("hypotheses", ctypes.c_uint32), ("degenerate", ctypes.c_uint32),
                ("found", ctypes.c_uint32), ("best", ctypes.c_uint32), ("triple", ctypes.c_uint32 * 3), ("inliers", ctypes.c_uint32),
                ("tests", ctypes.c_uint64), ("budget", ctypes.c_uint64), ("plane", ctypes.c_double * 4)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k not in ("triple", "plane")}
        d["triple"] = tuple(int(v) for v in self.triple)
        d["plane"] = np.array(self.plane, dtype=np.float64)
        return d


class GsrMatchInfo(ctypes.Structure):
    _fields_ = [("in_scope", ctypes.c_uint32), ("nonfinite", ctypes.c_uint32), ("target_indexed", ctypes.c_uint32), ("matched", ctypes.c_uint32),
                ("pair_bound", ctypes.c_uint64), ("budget", ctypes.c_uint64), ("d2_min", ctypes.c_double), ("d2_max", ctypes.c_double)]

    def as_dict(self):
        return {k: (float if t is ctypes.c_double else int)(getattr(self, k)) for k, t in self._fields_}


class GsrMatchSums(ctypes.Structure):
    _fields_ = [("pairs", ctypes.c_uint64), ("sum", ctypes.c_double * 16)]

    def as_dict(self):
        return {"pairs": int(self.pairs), "sum": np.array(self.sum, dtype=np.float64)}


class GsrRegisterInfo(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("iterations", ctypes.c_uint32), ("pairs", ctypes.c_uint64), ("rms", ctypes.c_double), ("delta", ctypes.c_double),
                ("step_pairs", ctypes.c_void_p), ("step_rms", ctypes.c_void_p), ("step_rows", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self):
        return {"status": REGISTER_STATUS[self.status], "iterations": int(self.iterations), "pairs": int(self.pairs), "rms": float(self.rms),
                "delta": float(self.delta)}


class GsrSurfaceSums(ctypes.Structure):
    _fields_ = [("pairs", ctypes.c_uint64), ("surface_pairs", ctypes.c_uint64), ("sum", ctypes.c_double * 29)]

    def as_dict(self):
        return {"pairs": int(self.pairs), "surface_pairs": int(self.surface_pairs), "sum": np.array(self.sum, dtype=np.float64)}


class GsrRegisterSurfaceInfo(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("iterations", ctypes.c_uint32), ("pairs", ctypes.c_uint64), ("surface_pairs", ctypes.c_uint64),
                ("rms", ctypes.c_double), ("surface_rms", ctypes.c_double), ("delta", ctypes.c_double), ("valid", ctypes.c_uint32), ("step_rows", ctypes.c_uint32),
                ("step_pairs", ctypes.c_void_p), ("step_surface_pairs", ctypes.c_void_p), ("step_rms", ctypes.c_void_p), ("step_surface_rms", ctypes.c_void_p)]

    def as_dict(self):
        return {"status": REGISTER_SURFACE_STATUS[self.status], "iterations": int(self.iterations), "pairs": int(self.pairs),
                "surface_pairs": int(self.surface_pairs), "rms": float(self.rms), "surface_rms": float(self.surface_rms), "delta": float(self.delta),
                "valid": int(self.valid)}


class GsrDepthLayout(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int32), ("step", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("reserved", ctypes.c_int32), ("offset", ctypes.c_uint64), ("bytes", ctypes.c_uint64),
                ("near", ctypes.c_float), ("reserved2", ctypes.c_int32)]


GSR_FORMAT_RGBA8, GSR_FORMAT_NV12, GSR_FORMAT_I420 = 0, 1, 2
DELIVERY_FORMATS = {"rgba8": GSR_FORMAT_RGBA8, "nv12": GSR_FORMAT_NV12, "i420": GSR_FORMAT_I420}
GSR_DEPTH_NONE, GSR_DEPTH_F32, GSR_DEPTH_U16 = 0, 1, 2
DEPTH_DELIVERY_FORMATS = {"f32": GSR_DEPTH_F32, "u16": GSR_DEPTH_U16}
OUTLINE_SIDES = {"outer": 0, "inner": 1}                                   # GSR_OUTLINE_*
SELECT_MODES = {"centre": 0, "hit": 1}                                     # GSR_SELECT_*
SELECT_OPS = {"replace": 0, "add": 1, "subtract": 2, "intersect": 3}       # GSR_SELOP_*
CONTRIB_STATS = {"weight": 0, "peak": 1, "pixels": 2}                      # GSR_CONTRIB_*
ATTRS = {"x": 0, "y": 1, "z": 2, "distance": 3, "red": 4, "green": 5, "blue": 6, "opacity": 7, "scale_x": 8, "scale_y": 9, "scale_z": 10,
         "scale_min": 11, "scale_max": 12, "contrib_weight": 13, "contrib_peak": 14, "contrib_pixels": 15}   # GSR_ATTR_*
SCOPES = {"selected": 1, "visible": 2}                                     # GSR_SCOPE_*
ATTR_MAX_BINS = 4096
NEIGHBOUR_MAX_CAP = 4095                                                   # GSR_NEIGHBOUR_MAX_CAP
NEIGHBOUR_DEFAULT_BUDGET, NEIGHBOUR_MAX_BUDGET = 1 << 34, 1 << 38          # GSR_NEIGHBOUR_*_BUDGET
KNN_MAX_K, KNN_NONE = 32, 0xffffffff                                       # GSR_KNN_MAX_K, GSR_KNN_NONE (an empty list slot)
KNN_STATS = {"kth": 0, "mean": 1}                                          # GSR_KNN_*
NORMAL_SOURCES = {"knn": 0, "own": 1}                                      # GSR_NORMAL_KNN / GSR_NORMAL_OWN
NORMAL_STATS = {"dot": 0, "abs_dot": 1, "variation": 2}                    # GSR_NORMAL_DOT / _ABS_DOT / _VARIATION
PLANE_MAX_HYPOTHESES = 4096                                               # GSR_PLANE_MAX_HYPOTHESES
MATCH_NONE = 0xffffffff                                                    # GSR_MATCH_NONE (an unmatched splat)
REGISTER_STATUS = {0: "converged", 1: "max_iterations", 2: "too_few"}      # GSR_REGISTER_*
REGISTER_SURFACE_STATUS = {**REGISTER_STATUS, 3: "degenerate"}             # with GSR_REGISTER_DEGENERATE (gsr_register_surface)
REGISTER_MAX_ITERATIONS = 256                                              # GSR_REGISTER_MAX_ITERATIONS_LIMIT
CELL_NONE = 0xffffffff                                                     # GSR_CELL_NONE (a leader: the splat is no candidate)
CLUSTER_NONE = CLUSTER_LARGEST = 0xffffffff                                # GSR_CLUSTER_NONE (a label), GSR_CLUSTER_LARGEST (a seed)


def knn_outlier_threshold(values, std_ratio):
    """The threshold of select_statistical_outliers, in f64: mu + std_ratio * sigma over the finite values, sigma the sample
    standard deviation (n - 1); +inf with fewer than two finite values."""
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    if v.size < 2:
        return float("inf")
    return float(np.mean(v) + np.float64(std_ratio) * np.std(v, ddof=1))


def plane_alignment(plane, axis=(0, 1, 0)):
    """(q_xyzw float64[4], t float64[3]) of gsr_plane_alignment: the rotation and translation that take `plane` (a, b, c, d) to
    axis . p = 0.  Needs the library, not a device."""
    L = load_library()
    p = np.ascontiguousarray(plane, dtype=np.float64).reshape(4)
    a = np.ascontiguousarray(axis, dtype=np.float64).reshape(3)
    q, t = np.zeros(4, np.float64), np.zeros(3, np.float64)
    rc = L.gsr_plane_alignment(p.ctypes.data, a.ctypes.data, q.ctypes.data, t.ctypes.data)
    if rc:
        err = GsplatError("libgsplat_hip error %d: %s" % (rc, L.gsr_last_error(None).decode()))
        err.code = rc
        raise err
    return q, t


def _pure(name, rc):
    if rc:
        err = GsplatError("libgsplat_hip error %d: %s" % (rc, load_library().gsr_last_error(None).decode()))
        err.code = rc
        raise err


def _transform_arg(transform):
    """a 3 x 4 transform (R | t) as twelve contiguous doubles, None for the identity"""
    return None if transform is None else np.ascontiguousarray(transform, dtype=np.float64).reshape(12)


def rigid_solve(sums):
    """(D float64[3, 4], rms) of gsr_rigid_solve: the rigid motion that takes the matched source points closest to their targets
    (Horn's closed form on match()'s sums, a dict with "pairs" and "sum").  Needs the library, not a device."""
    L = load_library()
    s = GsrMatchSums()
    s.pairs = int(sums["pairs"])
    s.sum[:] = [float(v) for v in np.asarray(sums["sum"], dtype=np.float64).reshape(16)]
    D, rms = np.zeros(12, np.float64), ctypes.c_double(0.0)
    _pure("gsr_rigid_solve", L.gsr_rigid_solve(ctypes.byref(s), D.ctypes.data, ctypes.byref(rms)))
    return D.reshape(3, 4), rms.value


def surface_solve(sums):
    """(D float64[3, 4], rms, degenerate) of gsr_surface_solve: the small rigid motion that takes the matched source points closest
    to the target's surface along its normals (Cholesky on match_surface()'s sums, a dict with "surface_pairs" and "sum"; a Cayley
    step for the rotation).  degenerate = j + 1 when pivot j of the 6 x 6 system is not above its floor -- the residuals leave a
    direction free, as a target of one or two planes does: D is then the identity and rms None.  Needs the library, not a device."""
    L = load_library()
    s = GsrSurfaceSums()
    s.pairs = int(sums.get("pairs", sums["surface_pairs"]))
    s.surface_pairs = int(sums["surface_pairs"])
    s.sum[:] = [float(v) for v in np.asarray(sums["sum"], dtype=np.float64).reshape(29)]
    D, rms, deg = np.zeros(12, np.float64), ctypes.c_double(0.0), ctypes.c_int32(0)
    _pure("gsr_surface_solve", L.gsr_surface_solve(ctypes.byref(s), D.ctypes.data, ctypes.byref(rms), ctypes.byref(deg)))
    return D.reshape(3, 4), (None if deg.value else rms.value), deg.value


def rigid_compose(D, M):
    """float64[3, 4] of gsr_rigid_compose: D o M, "apply M, then D"."""
    L = load_library()
    d, m, out = _transform_arg(D), _transform_arg(M), np.zeros(12, np.float64)
    _pure("gsr_rigid_compose", L.gsr_rigid_compose(d.ctypes.data, m.ctypes.data, out.ctypes.data))
    return out.reshape(3, 4)


def rigid_decompose(M):
    """(q_xyzw float64[4], t float64[3]) of gsr_rigid_decompose: scene_rotate(q) then scene_translate(t) applies the transform M
    to a scene."""
    L = load_library()
    m, q, t = _transform_arg(M), np.zeros(4, np.float64), np.zeros(3, np.float64)
    _pure("gsr_rigid_decompose", L.gsr_rigid_decompose(m.ctypes.data, q.ctypes.data, t.ctypes.data))
    return q, t


def sh_rotation(q_xyzw):
    """(D_1 float64[3, 3], D_2 float64[5, 5], D_3 float64[7, 7]) of gsr_sh_rotation: the band matrices that rotate SH coefficients
    by the rotation of q = (x, y, z, w) (finite, not zero; normalised in f64).  Needs the library, not a device."""
    L = load_library()
    q = np.ascontiguousarray(q_xyzw, dtype=np.float64).reshape(4)
    m = np.zeros(83, np.float64)
    _pure("gsr_sh_rotation", L.gsr_sh_rotation(q.ctypes.data, m.ctypes.data))
    return m[:9].reshape(3, 3), m[9:34].reshape(5, 5), m[34:].reshape(7, 7)


def attr_edges(lo, hi, bins):
    """The bins + 1 edges of gsr_attr_histogram, by the header's f64 rule: w = (hi - lo) / bins, edge(k) = min(lo + k * w, hi) and
    edge(bins) = hi.  select_attr(attr, edges[a], edges[b]) selects exactly sum(counts[a:b]) splats."""
    lo, hi = np.float64(lo), np.float64(hi)
    w = (hi - lo) / np.float64(bins)
    e = np.minimum(lo + np.arange(bins + 1, dtype=np.float64) * w, hi)
    e[bins] = hi
    return e


def edge_arrays(edges):
    """[(x0, x1)] per rank -> (c_int32[world], c_int32[world]) for gsr_unpack_slabs_rgba8_async."""
    world = len(edges)
    return ((ctypes.c_int32 * world)(*[int(a) for a, _ in edges]), (ctypes.c_int32 * world)(*[int(b) for _, b in edges]))


class GsplatError(RuntimeError):
    """`code`: the library's return code (GSR_ERR_*), None for errors raised by the harness itself."""
    code = None


_lib = None

# every symbol include/gsplat_hip.h declares
EXPORTS = [
    "gsr_create", "gsr_destroy", "gsr_last_error", "gsr_set_scene", "gsr_set_scene_sh", "gsr_read_sh_colors", "gsr_set_depth_fade", "gsr_resize",
    "gsr_set_scene_rows", "gsr_scene_translate", "gsr_scene_rotate", "gsr_scene_scale", "gsr_scene_limit_box", "gsr_read_scene", "gsr_set_band", "gsr_set_camera",
    "gsr_sort", "gsr_render", "gsr_render_async", "gsr_sync", "gsr_read_depth_index", "gsr_read_pixels_rgba32f",
    "gsr_read_pixels_rgba8", "gsr_get_timings", "gsr_reset_timings", "gsr_set_timing_interval", "gsr_read_keys", "gsr_read_records",
    "gsr_read_bin_totals", "gsr_read_bin_lists", "gsr_convert_rgba8_async", "gsr_framebuffer8_device_ptr",
    "gsr_pack_band_rgba8_async", "gsr_unpack_slabs_rgba8_async",
    "gsr_framebuffer_device_ptr", "gsr_stream_handle", "gsr_stream_order", "gsr_device_info", "gsplat_sort_host",
    "gsr_overflow_pending", "gsr_set_list_capacity", "gsr_scene_count", "gsr_build_id",
    "gsr_comm_unique_id", "gsr_comm_init", "gsr_comm_destroy", "gsr_allgather_frame_async", "gsr_read_frame_rgba8",
    "gsr_frame8_device_ptr", "gsr_comm_stream_handle", "gsr_read_work_items", "gsr_comm_share", "gsr_comm_init_custom",
    "gsr_delivery_open", "gsr_delivery_close", "gsr_deliver_frame_async", "gsr_frame_ready", "gsr_acquire_frame",
    "gsr_release_frame", "gsr_delivery_slot_ptr", "gsr_delivery_open_ex", "gsr_delivery_layout",
    "gsr_delivery_open_depth", "gsr_delivery_depth_layout",
    "gsr_set_hit_alpha", "gsr_depth_async", "gsr_read_depth", "gsr_depth_device_ptr", "gsr_pick",
    "gsr_set_scene_arrays",
    "gsr_comm_set_depth", "gsr_frame_depth_layout", "gsr_read_frame_depth", "gsr_frame_depth_device_ptr",
    "gsr_set_sh_follow", "gsr_set_sh_frame", "gsr_get_sh_frame", "gsr_read_scene_sh",
    "gsr_share_scene", "gsr_scene_sharing",
    "gsr_select_region", "gsr_select_box", "gsr_selection_set", "gsr_selection_invert", "gsr_read_selection", "gsr_scene_erase_selected",
    "gsr_hide_selected", "gsr_hidden_set", "gsr_read_hidden", "gsr_select_hidden",
    "gsr_selection_bounds", "gsr_scene_translate_selected", "gsr_scene_rotate_selected", "gsr_scene_scale_selected", "gsr_scene_set_rgba_selected",
    "gsr_sh_rotation", "gsr_scene_rotate_sh", "gsr_scene_rotate_selected_sh", "gsr_scene_bake_sh_frame",
    "gsr_scene_reserve", "gsr_scene_capacity", "gsr_scene_duplicate_selected", "gsr_scene_append_selected", "gsr_scene_append_arrays",
    "gsr_contrib_reset", "gsr_contrib_accumulate_async", "gsr_read_contrib", "gsr_select_contrib",
    "gsr_attr_stats", "gsr_attr_histogram", "gsr_select_attr",
    "gsr_neighbours", "gsr_select_neighbours",
    "gsr_clusters", "gsr_select_clusters", "gsr_select_cluster_at",
    "gsr_knn", "gsr_select_knn",
    "gsr_cells", "gsr_scene_merge_cells",
    "gsr_fit_plane", "gsr_plane_inliers", "gsr_select_plane", "gsr_plane_alignment",
    "gsr_match", "gsr_select_match", "gsr_register", "gsr_rigid_solve", "gsr_rigid_compose", "gsr_rigid_decompose",
    "gsr_normals", "gsr_select_normal",
    "gsr_match_surface", "gsr_surface_solve", "gsr_register_surface",
    "gsr_set_overlay", "gsr_overlay_async", "gsr_read_overlay", "gsr_read_overlay_rgba8", "gsr_overlay_device_ptr", "gsr_delivery_set_overlay",
    "gsr_set_overlay_outline",
]
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p)
GSR_COMM_ID_BYTES = 128
GSR_SH_ALL, GSR_SH_SELECTED = 0, 1   # gsr_scene_rotate_sh's scope
PICK_DTYPE = np.dtype([("index", np.uint32), ("depth", np.float32), ("mean", np.float32), ("alpha", np.float32)])   # gsr_pick_result


def _assert_one_hip_runtime():
    """The library and torch must share ONE libamdhip64 (streams, events and device pointers cross between them).
    Which copy that is depends on load order (see load_library); two mapped copies mean two runtimes in the process,
    which fails in obscure ways later, so fail here with the reason."""
    try:
        with open("/proc/self/maps") as f:
            paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    except OSError:
        return
    if len(paths) > 1:
        raise GsplatError("two HIP runtimes are mapped into this process (%s): import torch before gsplat_hip, or set "
                          "GSPLAT_HIP_NO_TORCH=1 in a process that never uses torch" % ", ".join(sorted(paths)))


def load_library(path=None):
    """Load libgsplat_hip.so and declare its prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("GSPLAT_HIP_LIB") or LIB_PATH   # GSPLAT_HIP_LIB: experiment builds
    if not os.path.exists(p):
        raise GsplatError("libgsplat_hip.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`" % p)
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as the system one
    # this library links against).  If torch is imported first, the loader gives this library torch's copy and the two
    # share streams, events and memory (the N>1 exchange relies on that); loaded the other way round, the process ends
    # up with two runtimes and torch cannot see the GPU any more.  So: when torch is installed, import it before the
    # library (GSPLAT_HIP_NO_TORCH=1 skips this for hosts that never touch torch).
    import sys
    if "torch" not in sys.modules and os.environ.get("GSPLAT_HIP_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = ctypes.CDLL(p)
    _assert_one_hip_runtime()
    vp = ctypes.c_void_p
    L.gsr_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(GsrOptions)]
    L.gsr_destroy.argtypes = [vp]
    L.gsr_last_error.argtypes = [vp]
    L.gsr_last_error.restype = ctypes.c_char_p
    L.gsr_set_scene.argtypes = [vp, vp, vp, ctypes.c_uint32]
    L.gsr_set_scene_sh.argtypes = [vp, vp, vp, vp, ctypes.c_uint32, vp]
    L.gsr_read_sh_colors.argtypes = [vp, vp]
    L.gsr_set_depth_fade.argtypes = [vp, ctypes.c_int32, ctypes.c_float]
    L.gsr_set_scene_rows.argtypes = [vp, vp, ctypes.c_uint32]
    L.gsr_set_scene_arrays.argtypes = [vp, vp, vp, vp, vp, ctypes.c_uint32]
    for name in ("gsr_scene_translate", "gsr_scene_rotate", "gsr_scene_scale"):
        getattr(L, name).argtypes = [vp, vp]
    L.gsr_scene_limit_box.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_uint32)]
    L.gsr_read_scene.argtypes = [vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_uint32)]
    L.gsr_resize.argtypes = [vp, ctypes.c_int32, ctypes.c_int32]
    L.gsr_set_band.argtypes = [vp, ctypes.c_int32, ctypes.c_int32]
    L.gsr_set_camera.argtypes = [vp, vp, vp, vp, ctypes.c_float, ctypes.c_float]
    for name in ("gsr_sort", "gsr_render", "gsr_render_async", "gsr_sync", "gsr_reset_timings"):
        getattr(L, name).argtypes = [vp]
    L.gsr_read_depth_index.argtypes = [vp, vp]
    L.gsr_read_pixels_rgba32f.argtypes = [vp, vp]
    L.gsr_read_pixels_rgba8.argtypes = [vp, vp]
    L.gsr_get_timings.argtypes = [vp, ctypes.POINTER(GsrTimings)]
    L.gsr_set_timing_interval.argtypes = [vp, ctypes.c_uint32]
    L.gsr_read_keys.argtypes = [vp, vp, vp]
    L.gsr_read_records.argtypes = [vp, vp, vp]
    L.gsr_read_bin_totals.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.gsr_read_bin_lists.argtypes = [vp, vp, vp, ctypes.c_uint64]
    L.gsr_convert_rgba8_async.argtypes = [vp]
    L.gsr_read_work_items.argtypes = [vp, vp]
    L.gsr_stream_order.argtypes = [vp, vp, ctypes.c_int32]
    L.gsr_pack_band_rgba8_async.argtypes = [vp, vp, ctypes.c_int32]
    L.gsr_unpack_slabs_rgba8_async.argtypes = [vp, vp, vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                               ctypes.POINTER(ctypes.c_int32), vp]
    L.gsr_framebuffer8_device_ptr.argtypes = [vp]
    L.gsr_framebuffer8_device_ptr.restype = vp
    L.gsr_framebuffer_device_ptr.argtypes = [vp]
    L.gsr_framebuffer_device_ptr.restype = vp
    L.gsr_stream_handle.argtypes = [vp]
    L.gsr_stream_handle.restype = vp
    L.gsr_device_info.argtypes = [vp, ctypes.c_char_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                  ctypes.POINTER(ctypes.c_int32)]
    L.gsplat_sort_host.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp]
    L.gsplat_sort_host.restype = None
    L.gsr_overflow_pending.argtypes = [vp]
    L.gsr_set_list_capacity.argtypes = [vp, ctypes.c_uint32]
    L.gsr_scene_count.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    L.gsr_build_id.argtypes = []
    L.gsr_build_id.restype = ctypes.c_char_p
    L.gsr_comm_unique_id.argtypes = [vp]
    L.gsr_comm_init.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.gsr_comm_share.argtypes = [vp, vp]
    L.gsr_comm_init_custom.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                       ALLGATHER_FN, vp]
    L.gsr_comm_destroy.argtypes = [vp]
    L.gsr_allgather_frame_async.argtypes = [vp]
    L.gsr_read_frame_rgba8.argtypes = [vp, vp]
    L.gsr_frame8_device_ptr.argtypes = [vp]
    L.gsr_frame8_device_ptr.restype = vp
    L.gsr_comm_stream_handle.argtypes = [vp]
    L.gsr_comm_stream_handle.restype = vp
    L.gsr_delivery_open.argtypes = [vp, ctypes.c_int32]
    L.gsr_delivery_close.argtypes = [vp]
    L.gsr_deliver_frame_async.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.gsr_frame_ready.argtypes = [vp, ctypes.c_uint64]
    L.gsr_acquire_frame.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(GsrFrame)]
    L.gsr_release_frame.argtypes = [vp, ctypes.c_uint64]
    L.gsr_delivery_slot_ptr.argtypes = [vp, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)]
    L.gsr_delivery_slot_ptr.restype = vp
    L.gsr_delivery_open_ex.argtypes = [vp, ctypes.POINTER(GsrDeliveryOptions)]
    L.gsr_delivery_layout.argtypes = [vp, ctypes.POINTER(GsrFrameLayout)]
    L.gsr_delivery_open_depth.argtypes = [vp, ctypes.POINTER(GsrDeliveryOptions), ctypes.POINTER(GsrDepthDeliveryOptions)]
    L.gsr_delivery_depth_layout.argtypes = [vp, ctypes.POINTER(GsrDepthLayout)]
    L.gsr_set_hit_alpha.argtypes = [vp, ctypes.c_float]
    L.gsr_depth_async.argtypes = [vp]
    L.gsr_read_depth.argtypes = [vp, vp, vp, vp]
    L.gsr_depth_device_ptr.argtypes = [vp, ctypes.c_int32]
    L.gsr_depth_device_ptr.restype = vp
    L.gsr_pick.argtypes = [vp, vp, ctypes.c_uint32, vp]
    L.gsr_comm_set_depth.argtypes = [vp, ctypes.POINTER(GsrDepthDeliveryOptions)]
    L.gsr_frame_depth_layout.argtypes = [vp, ctypes.POINTER(GsrDepthLayout)]
    L.gsr_read_frame_depth.argtypes = [vp, vp, ctypes.c_uint64]
    L.gsr_frame_depth_device_ptr.argtypes = [vp]
    L.gsr_frame_depth_device_ptr.restype = vp
    L.gsr_set_sh_follow.argtypes = [vp, ctypes.c_int32]
    L.gsr_set_sh_frame.argtypes = [vp, vp]
    L.gsr_get_sh_frame.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_int32)]
    L.gsr_read_scene_sh.argtypes = [vp, vp, vp, vp, ctypes.POINTER(ctypes.c_uint32), vp]
    L.gsr_share_scene.argtypes = [vp, vp]
    L.gsr_scene_sharing.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)]
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.gsr_select_region.argtypes = [vp, ctypes.POINTER(GsrRegion), ctypes.c_int32, ctypes.c_int32, u32p]
    L.gsr_select_box.argtypes = [vp, vp, ctypes.c_int32, u32p]
    L.gsr_selection_set.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_int32, u32p]
    L.gsr_selection_invert.argtypes = [vp, u32p]
    L.gsr_read_selection.argtypes = [vp, vp, ctypes.c_uint32, u32p]
    L.gsr_scene_erase_selected.argtypes = [vp, ctypes.c_int32, u32p]
    L.gsr_hide_selected.argtypes = [vp, ctypes.c_int32, u32p]
    L.gsr_hidden_set.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_int32, u32p]
    L.gsr_read_hidden.argtypes = [vp, vp, ctypes.c_uint32, u32p]
    L.gsr_select_hidden.argtypes = [vp, ctypes.c_int32, u32p]
    L.gsr_selection_bounds.argtypes = [vp, ctypes.POINTER(GsrSelectionBounds)]
    L.gsr_scene_translate_selected.argtypes = [vp, vp]
    L.gsr_scene_rotate_selected.argtypes = [vp, vp, vp]
    L.gsr_sh_rotation.argtypes = [vp, vp]
    L.gsr_scene_rotate_sh.argtypes = [vp, vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    L.gsr_scene_rotate_selected_sh.argtypes = [vp, vp, vp]
    L.gsr_scene_bake_sh_frame.argtypes = [vp, vp]
    L.gsr_scene_scale_selected.argtypes = [vp, vp, vp]
    L.gsr_scene_set_rgba_selected.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32]
    L.gsr_scene_reserve.argtypes = [vp, ctypes.c_uint32]
    L.gsr_scene_capacity.argtypes = [vp, u32p]
    L.gsr_scene_duplicate_selected.argtypes = [vp, u32p, u32p]
    L.gsr_scene_append_selected.argtypes = [vp, vp, u32p, u32p]
    L.gsr_scene_append_arrays.argtypes = [vp, vp, vp, vp, vp, ctypes.c_uint32, u32p]
    L.gsr_contrib_reset.argtypes = [vp]
    L.gsr_contrib_accumulate_async.argtypes = [vp]
    L.gsr_read_contrib.argtypes = [vp, vp, vp, vp, ctypes.c_uint32, u32p]
    L.gsr_select_contrib.argtypes = [vp, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, u32p]
    f64p = ctypes.POINTER(ctypes.c_double)
    L.gsr_attr_stats.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_uint32, u32p, u32p, f64p, f64p]
    L.gsr_attr_histogram.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_uint32, vp, vp]
    L.gsr_select_attr.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_double, ctypes.c_double, ctypes.c_int32, u32p]
    u64 = ctypes.c_uint64
    L.gsr_neighbours.argtypes = [vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, vp, ctypes.c_uint32, vp, ctypes.POINTER(GsrNeighbourInfo)]
    L.gsr_select_neighbours.argtypes = [vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32, u32p,
                                        ctypes.POINTER(GsrNeighbourInfo)]
    ci = ctypes.POINTER(GsrClusterInfo)
    L.gsr_clusters.argtypes = [vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, vp, vp, ctypes.c_uint32, ci]
    L.gsr_select_clusters.argtypes = [vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32, u32p, ci]
    L.gsr_select_cluster_at.argtypes = [vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, ctypes.c_uint32, ctypes.c_int32, u32p, ci]
    ki = ctypes.POINTER(GsrKnnInfo)
    L.gsr_knn.argtypes = [vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, ctypes.c_int32, vp, vp, vp, vp, ctypes.c_uint32, vp, ki]
    L.gsr_select_knn.argtypes = [vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32, u32p, ki]
    gi = ctypes.POINTER(GsrCellInfo)
    L.gsr_cells.argtypes = [vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, vp, ctypes.c_uint32, vp, gi]
    L.gsr_scene_merge_cells.argtypes = [vp, ctypes.c_double, ctypes.c_uint32, u64, u32p, gi]
    pi = ctypes.POINTER(GsrPlaneInfo)
    L.gsr_fit_plane.argtypes = [vp, ctypes.c_double, ctypes.c_uint32, u64, ctypes.c_uint32, u64, vp, pi]
    L.gsr_plane_inliers.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_double, ctypes.c_uint32, u64, vp, pi]
    L.gsr_select_plane.argtypes = [vp, vp, ctypes.c_double, ctypes.c_double, ctypes.c_int32, u32p]
    L.gsr_plane_alignment.argtypes = [vp, vp, vp, vp]
    mi = ctypes.POINTER(GsrMatchInfo)
    L.gsr_match.argtypes = [vp, vp, vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, vp, vp, ctypes.c_uint32, ctypes.POINTER(GsrMatchSums), mi]
    L.gsr_select_match.argtypes = [vp, vp, vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, ctypes.c_double, ctypes.c_double, ctypes.c_int32, u32p, mi]
    L.gsr_register.argtypes = [vp, vp, vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, ctypes.c_uint32, ctypes.c_double, vp, ctypes.POINTER(GsrRegisterInfo)]
    L.gsr_rigid_solve.argtypes = [ctypes.POINTER(GsrMatchSums), vp, ctypes.POINTER(ctypes.c_double)]
    L.gsr_rigid_compose.argtypes = [vp, vp, vp]
    L.gsr_rigid_decompose.argtypes = [vp, vp, vp]
    no, nmi = ctypes.POINTER(GsrNormalOptions), ctypes.POINTER(GsrNormalInfo)
    L.gsr_normals.argtypes = [vp, no, vp, vp, vp, ctypes.c_uint32, nmi]
    L.gsr_select_normal.argtypes = [vp, no, ctypes.c_int32, vp, ctypes.c_double, ctypes.c_double, ctypes.c_int32, u32p, nmi]
    L.gsr_match_surface.argtypes = [vp, vp, vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, no, ctypes.POINTER(GsrSurfaceSums), mi]
    L.gsr_surface_solve.argtypes = [ctypes.POINTER(GsrSurfaceSums), vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    L.gsr_register_surface.argtypes = [vp, vp, vp, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, u64, no, ctypes.c_uint32, ctypes.c_double, vp,
                                       ctypes.POINTER(GsrRegisterSurfaceInfo)]
    L.gsr_set_overlay.argtypes = [vp, ctypes.POINTER(GsrOverlayOptions)]
    L.gsr_set_overlay_outline.argtypes = [vp, ctypes.POINTER(GsrOutlineOptions)]
    L.gsr_overlay_async.argtypes = [vp]
    L.gsr_read_overlay.argtypes = [vp, vp, vp]
    L.gsr_read_overlay_rgba8.argtypes = [vp, vp]
    L.gsr_overlay_device_ptr.argtypes = [vp, ctypes.c_int32]
    L.gsr_overlay_device_ptr.restype = vp
    L.gsr_delivery_set_overlay.argtypes = [vp, ctypes.c_int32]
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is ctypes.c_int and name not in ("gsplat_sort_host",):
            fn.restype = ctypes.c_int
    if path is None:
        _lib = L
    return L


# ---------------------------------------------------------------------------
# Scene: mirror of src/core/Scene.ts (setData only: the producer of the buffers
# the hot path consumes), vectorised in numpy float64 = JS number arithmetic.
# ---------------------------------------------------------------------------
def _float_to_half(x64):
    """src/utils.ts:16-43 (truncating; JS `>>` shift count taken modulo 32)."""
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.asarray(x64, dtype=np.float64).astype(np.float32).view(np.int32).astype(np.int64)
    sign = (f >> 31) & 1
    exp = (f >> 23) & 0xFF
    frac = f & 0x007FFFFF
    sub = (exp > 0) & (exp < 113)
    shift = np.where(sub, (113 - exp) & 31, 0)
    frac_sub = (frac | 0x00800000) >> shift
    carry = sub & ((frac_sub & 0x01000000) != 0)
    new_exp = np.where(exp == 0, 0, np.where(exp < 113, 0, np.where(exp < 142, exp - 112, 31)))
    new_exp = np.where(carry, 1, new_exp)
    frac_out = np.where(sub, frac_sub, frac)
    frac_out = np.where(carry | (exp >= 142), 0, frac_out)
    return ((sign << 15) | (new_exp << 10) | (frac_out >> 13)).astype(np.uint32)


def pack_half2x16(x, y):
    """src/utils.ts:46-48."""
    return (_float_to_half(x) | (_float_to_half(y) << np.uint32(16))).astype(np.uint32)


class Scene:
    RowLength = 32  # src/core/Scene.ts:9

    def __init__(self):
        self._listeners = {}
        self.data = np.zeros(0, dtype=np.uint32)
        self.positions = np.zeros(0, dtype=np.float32)
        self.vertexCount = 0
        self.width = 2048
        self.height = 0
        self.shHeight = 0
        self.shs_rgb = [np.zeros(0, dtype=np.uint32) for _ in range(3)]
        self.bandsIndices = np.array([-1, -1, -1], dtype=np.int32)

    # EventDispatcher surface used by the renderer (src/core/EventDispatcher.ts)
    def addEventListener(self, kind, fn):
        self._listeners.setdefault(kind, []).append(fn)

    def removeEventListener(self, kind, fn):
        if fn in self._listeners.get(kind, []):
            self._listeners[kind].remove(fn)

    def dispatchEvent(self, kind):
        for fn in list(self._listeners.get(kind, [])):
            fn({"type": kind})

    def setData(self, rows, shs=None):
        """Scene.ts:58-180.  shs: 48 floats per SH-carrying splat (set bandsIndices first, like the loader does)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1)
        if rows.size % self.RowLength:
            raise ValueError("data length must be a multiple of %d" % self.RowLength)
        n = rows.size // self.RowLength
        self.vertexCount = n
        self.height = -(-(2 * n) // self.width)
        r = rows.reshape(n, 32)
        f = r[:, :24].copy().view(np.float32).reshape(n, 6)
        self.positions = f[:, 0:3].copy().reshape(-1)
        data = np.zeros((self.width * self.height * 4) if n else 0, dtype=np.uint32)
        d = data[:8 * n].reshape(n, 8)
        d[:, 0:3] = f[:, 0:3].copy().view(np.uint32)
        d[:, 7] = r[:, 24:28].copy().view(np.uint32).reshape(n)
        rot = (r[:, 28:32].astype(np.float64) - 128.0) / 128.0
        qx, qy, qz, qw = rot[:, 1], rot[:, 2], rot[:, 3], -rot[:, 0]
        R = [1 - 2 * qy * qy - 2 * qz * qz, 2 * qx * qy - 2 * qz * qw, 2 * qx * qz + 2 * qy * qw,
             2 * qx * qy + 2 * qz * qw, 1 - 2 * qx * qx - 2 * qz * qz, 2 * qy * qz - 2 * qx * qw,
             2 * qx * qz - 2 * qy * qw, 2 * qy * qz + 2 * qx * qw, 1 - 2 * qx * qx - 2 * qy * qy]
        s = f[:, 3:6].astype(np.float64)
        z = np.zeros(n)
        a = [s[:, 0], z, z, z, s[:, 1], z, z, z, s[:, 2]]
        b = R
        M = [b[0] * a[0] + b[3] * a[1] + b[6] * a[2], b[1] * a[0] + b[4] * a[1] + b[7] * a[2], b[2] * a[0] + b[5] * a[1] + b[8] * a[2],
             b[0] * a[3] + b[3] * a[4] + b[6] * a[5], b[1] * a[3] + b[4] * a[4] + b[7] * a[5], b[2] * a[3] + b[5] * a[4] + b[8] * a[5],
             b[0] * a[6] + b[3] * a[7] + b[6] * a[8], b[1] * a[6] + b[4] * a[7] + b[7] * a[8], b[2] * a[6] + b[5] * a[7] + b[8] * a[8]]
        sg = [M[0] * M[0] + M[3] * M[3] + M[6] * M[6], M[0] * M[1] + M[3] * M[4] + M[6] * M[7],
              M[0] * M[2] + M[3] * M[5] + M[6] * M[8], M[1] * M[1] + M[4] * M[4] + M[7] * M[7],
              M[1] * M[2] + M[4] * M[5] + M[7] * M[8], M[2] * M[2] + M[5] * M[5] + M[8] * M[8]]
        d[:, 4] = pack_half2x16(4 * sg[0], 4 * sg[1])
        d[:, 5] = pack_half2x16(4 * sg[2], 4 * sg[3])
        d[:, 6] = pack_half2x16(4 * sg[4], 4 * sg[5])
        self.data = data
        if shs is not None:   # Scene.ts:83-124: three half textures, one per colour channel
            shs = np.ascontiguousarray(shs, dtype=np.float32).reshape(-1)
            count = n - (int(self.bandsIndices[0]) + 1)
            self.shHeight = -(-(2 * count) // self.width)
            c = shs[:count * 48].reshape(count, 8, 2, 3).astype(np.float64)   # (splat, word, half, channel)
            self.shs_rgb = []
            for ch in range(3):
                tex = np.zeros(self.width * self.shHeight * 4, dtype=np.uint32)
                tex[:8 * count] = pack_half2x16(c[:, :, 0, ch].reshape(-1), c[:, :, 1, ch].reshape(-1))
                self.shs_rgb.append(tex)
        else:
            self.shHeight = 0
        self.dispatchEvent("change")


# ---------------------------------------------------------------------------
# HIPRenderer: the drop-in for WebGLRenderer's render path
# ---------------------------------------------------------------------------
class HIPRenderer:
    """renderer.render(scene, camera) on an MI355X (WebGLRenderer.ts:241-296)."""

    def __init__(self, width=1920, height=1080, device=0, early_out_eps=0.0, band=None, timing=False, lib_path=None,
                 throughput=False):
        self._L = load_library(lib_path)
        self._ctx = ctypes.c_void_p()
        opt = GsrOptions(device, width, height, early_out_eps, band[0] if band else 0, band[1] if band else 0,
                         (GSR_FLAG_TIMING if timing else 0) | (GSR_FLAG_THROUGHPUT if throughput else 0))
        rc = self._L.gsr_create(ctypes.byref(self._ctx), ctypes.byref(opt))
        if rc:
            raise GsplatError("gsr_create failed (%d): %s" % (rc, self._L.gsr_last_error(None).decode()))
        self.width, self.height = width, height
        self._scene = None
        self._camera = None
        self._n = 0
        self._slot_views = {}   # delivery slot -> [H, W, 4] uint8 view of its pinned block (a depth ring: that and the depth view)
        self._depth_ring = False
        self._shared = False    # this renderer has shared a scene: the count can change through another member (_count)
        self._on_change = lambda _e: self._upload(self._scene)

    # -- helpers --
    def _check(self, rc):
        if rc:
            err = GsplatError("libgsplat_hip error %d: %s" % (rc, self._L.gsr_last_error(self._ctx).decode()))
            err.code = rc
            raise err

    def _upload(self, scene):
        data = np.ascontiguousarray(scene.data, dtype=np.uint32)
        pos = np.ascontiguousarray(scene.positions, dtype=np.float32)
        self._check(self._L.gsr_set_scene(self._ctx, data.ctypes.data, pos.ctypes.data, scene.vertexCount))
        self._n = scene.vertexCount
        if getattr(scene, "shHeight", 0):   # WebGLRenderer.ts:202-211: SH textures + u_bandIndex only when the scene has them
            self.set_sh(scene.shs_rgb, scene.bandsIndices)

    # -- reference surface --
    def setSize(self, width, height):
        self._check(self._L.gsr_resize(self._ctx, width, height))
        self.width, self.height = width, height
        self._slot_views = {}   # (a ring of another size has new blocks)

    def set_band(self, x0, x1):
        self._check(self._L.gsr_set_band(self._ctx, x0, x1))

    def set_raw_scene(self, data, positions):
        """Upload Scene.data / Scene.positions arrays directly (no Scene object)."""
        data = np.ascontiguousarray(data, dtype=np.uint32)
        pos = np.ascontiguousarray(positions, dtype=np.float32)
        n = pos.size // 3
        self._check(self._L.gsr_set_scene(self._ctx, data.ctypes.data, pos.ctypes.data, n))
        self._n = n
        self._scene = None

    def set_sh(self, shs_rgb, bands_indices):
        band = np.ascontiguousarray(bands_indices, dtype=np.int32)
        count = self._count() - (int(band[0]) + 1)
        tex = [np.ascontiguousarray(t, dtype=np.uint32) for t in shs_rgb]
        self._check(self._L.gsr_set_scene_sh(self._ctx, tex[0].ctypes.data, tex[1].ctypes.data, tex[2].ctypes.data, count,
                                             band.ctypes.data))

    def read_sh_colors(self):
        out = np.empty((self._count(), 4), dtype=np.float32)
        self._check(self._L.gsr_read_sh_colors(self._ctx, out.ctypes.data))
        return out

    # -- SH colour that follows the scene's transforms (gsr_set_sh_follow) --
    def set_sh_follow(self, on):
        """While on, scene_rotate / scene_scale keep the SH frame up and scene_limit_box compacts the SH textures with the scene."""
        self._check(self._L.gsr_set_sh_follow(self._ctx, 1 if on else 0))

    def set_sh_frame(self, linv=None):
        """The SH frame (3x3 row-major float64; None: the identity) of the SH state set_sh uploaded."""
        if linv is None:
            self._check(self._L.gsr_set_sh_frame(self._ctx, None))
            return
        m = np.ascontiguousarray(linv, dtype=np.float64).reshape(-1)
        if m.size != 9:
            raise ValueError("the SH frame is 3x3")
        self._check(self._L.gsr_set_sh_frame(self._ctx, m.ctypes.data))

    def sh_frame(self):
        """(frame float64[3, 3], follow bool)"""
        m = np.zeros(9, dtype=np.float64)
        follow = ctypes.c_int32(0)
        self._check(self._L.gsr_get_sh_frame(self._ctx, m.ctypes.data, ctypes.byref(follow)))
        return m.reshape(3, 3), bool(follow.value)

    def read_scene_sh(self):
        """([sh_r, sh_g, sh_b] uint32[8 * sh_count] each, bandsIndices int32[3]) as the device holds them; sh_count 0: no SH state."""
        count = ctypes.c_uint32(0)
        band = np.zeros(3, dtype=np.int32)
        self._check(self._L.gsr_read_scene_sh(self._ctx, None, None, None, ctypes.byref(count), band.ctypes.data))
        tex = [np.zeros(8 * count.value, dtype=np.uint32) for _ in range(3)]
        if count.value:
            self._check(self._L.gsr_read_scene_sh(self._ctx, tex[0].ctypes.data, tex[1].ctypes.data, tex[2].ctypes.data, None, None))
        return tex, band

    # -- shared scenes (gsr_share_scene): several renderers of one GPU render from one device copy --
    def share_scene(self, other):
        """Give up this renderer's scene and render `other`'s from now on: the same device arrays, nothing copied or uploaded.
        Edits (scene_*), SH state and the count are then the members' together; set_scene_rows / set_raw_scene / set_scene_arrays
        take a renderer out of the share again."""
        self._check(self._L.gsr_share_scene(self._ctx, other._ctx))
        self._shared = other._shared = True
        if self._scene is not None:
            self._scene.removeEventListener("change", self._on_change)
            self._scene = None
        self._n = self.scene_count()

    def scene_sharing(self):
        """(members, scene_bytes): renderers that render this renderer's scene (1: not shared) and the device bytes they hold once."""
        members, nbytes = ctypes.c_int32(0), ctypes.c_uint64(0)
        self._check(self._L.gsr_scene_sharing(self._ctx, ctypes.byref(members), ctypes.byref(nbytes)))
        return members.value, int(nbytes.value)

    def _count(self):
        """The splat count read-backs are sized by: this renderer's own record, or the shared scene's (another member may have cut it)."""
        if self._shared and self._ctx:
            self._n = self.scene_count()
        return self._n

    # -- on-device scene build and transforms (Scene.ts:58-366 as kernels) --
    def set_scene_rows(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1)
        self._check(self._L.gsr_set_scene_rows(self._ctx, rows.ctypes.data, rows.size // 32))
        self._n = rows.size // 32
        self._scene = None

    def set_scene_arrays(self, data, positions, rotations, scales):
        """A device scene the transforms accept, from Scene.data / positions / rotations (w, x, y, z) / scales as they are."""
        data = np.ascontiguousarray(data, dtype=np.uint32).reshape(-1)
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1)
        rot = np.ascontiguousarray(rotations, dtype=np.float32).reshape(-1)
        scl = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
        n = pos.size // 3
        if data.size < 8 * n or rot.size != 4 * n or scl.size != 3 * n:
            raise ValueError("data / rotations / scales do not hold %d splats" % n)
        self._check(self._L.gsr_set_scene_arrays(self._ctx, data.ctypes.data, pos.ctypes.data, rot.ctypes.data, scl.ctypes.data, n))
        self._n = n
        self._scene = None

    def scene_translate(self, t):
        t = np.ascontiguousarray(t, dtype=np.float64)
        self._check(self._L.gsr_scene_translate(self._ctx, t.ctypes.data))

    def scene_rotate(self, q_xyzw):
        q = np.ascontiguousarray(q_xyzw, dtype=np.float64)
        self._check(self._L.gsr_scene_rotate(self._ctx, q.ctypes.data))

    def scene_scale(self, s):
        s = np.ascontiguousarray(s, dtype=np.float64)
        self._check(self._L.gsr_scene_scale(self._ctx, s.ctypes.data))

    def scene_limit_box(self, box):
        box = np.ascontiguousarray(box, dtype=np.float64)
        n = ctypes.c_uint32(0)
        self._check(self._L.gsr_scene_limit_box(self._ctx, box.ctypes.data, ctypes.byref(n)))
        self._n = n.value
        return n.value

    def read_scene(self, with_rows=True):
        """(data u32[8n], positions f32[3n], rotations f32[4n] | None, scales f32[3n] | None)"""
        n = self._count()
        data = np.zeros(8 * n, dtype=np.uint32)
        pos = np.zeros(3 * n, dtype=np.float32)
        rot = np.zeros(4 * n, dtype=np.float32) if with_rows else None
        scl = np.zeros(3 * n, dtype=np.float32) if with_rows else None
        cnt = ctypes.c_uint32(0)
        self._check(self._L.gsr_read_scene(self._ctx, data.ctypes.data, pos.ctypes.data, rot.ctypes.data if with_rows else None,
                                           scl.ctypes.data if with_rows else None, ctypes.byref(cnt)))
        assert cnt.value == n
        return data, pos, rot, scl

    def set_depth_fade(self, use, value):
        """u_useDepthFade / u_depthFade of FadeInPass."""
        self._check(self._L.gsr_set_depth_fade(self._ctx, 1 if use else 0, float(value)))

    def set_camera(self, camera):
        camera.update(self.width, self.height)
        v, p, vp = camera.f32()
        self._check(self._L.gsr_set_camera(self._ctx, v.ctypes.data, p.ctypes.data, vp.ctypes.data, camera.fx, camera.fy))
        self._camera = camera

    def set_camera_arrays(self, view, proj, view_proj, fx, fy):
        """Pre-rounded float32[16] matrices (what `new Float32Array(m.buffer)` yields)."""
        self._check(self._L.gsr_set_camera(self._ctx, view.ctypes.data, proj.ctypes.data, view_proj.ctypes.data, fx, fy))

    def render(self, scene, camera, sync=True):
        if scene is not None and scene is not self._scene:
            if self._scene is not None:
                self._scene.removeEventListener("change", self._on_change)
            self._scene = scene
            scene.addEventListener("change", self._on_change)
            self._upload(scene)
        self.set_camera(camera)
        self._check(self._L.gsr_render(self._ctx) if sync else self._L.gsr_render_async(self._ctx))

    def render_async(self):
        self._check(self._L.gsr_render_async(self._ctx))

    def sync(self):
        """Wait for the enqueued frames.  Raises GsplatError (code -5) once if asynchronous frames were lost to a list
        overflow; the lists have been regrown by then and the renderer stays usable."""
        self._check(self._L.gsr_sync(self._ctx))

    def overflow_pending(self):
        """True while the device has reported a list overflow that the host has not handled (no copy, no sync)."""
        return bool(self._L.gsr_overflow_pending(self._ctx))

    def set_list_capacity(self, entries):
        """Tuning/test hook: capacity of the bin-list buffer in entries (call after the scene is uploaded)."""
        self._check(self._L.gsr_set_list_capacity(self._ctx, int(entries)))

    def scene_count(self):
        n = ctypes.c_uint32(0)
        self._check(self._L.gsr_scene_count(self._ctx, ctypes.byref(n)))
        return n.value

    def sort(self, camera=None):
        if camera is not None:
            self.set_camera(camera)
        self._check(self._L.gsr_sort(self._ctx))

    def dispose(self):
        if self._ctx:
            self._slot_views = {}
            self._L.gsr_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass

    # -- results --
    def lastDepthIndex(self):
        out = np.empty(self._count(), dtype=np.uint32)
        self._check(self._L.gsr_read_depth_index(self._ctx, out.ctypes.data))
        return out

    def readPixelsFloat(self, out=None):
        """premultiplied RGBA float32 [H, W, 4], row 0 = top; `out` (C-contiguous, that shape and dtype) is filled and returned"""
        if out is None:
            out = np.empty((self.height, self.width, 4), dtype=np.float32)
        elif out.dtype != np.float32 or out.size != self.height * self.width * 4 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous float32 array of height*width*4 elements")
        self._check(self._L.gsr_read_pixels_rgba32f(self._ctx, out.ctypes.data))
        return out

    def readPixels(self, out=None):
        """RGBA8 [H, W, 4], row 0 = top; `out` (C-contiguous uint8, height*width*4 elements) is filled and returned"""
        if out is None:
            out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        elif out.dtype != np.uint8 or out.size != self.height * self.width * 4 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous uint8 array of height*width*4 elements")
        self._check(self._L.gsr_read_pixels_rgba8(self._ctx, out.ctypes.data))
        return out

    # -- frame delivery: frames through the library's pinned ring while the next frames render (gsr_delivery_*) --
    def open_delivery(self, slots=3, format="rgba8", full_range=False, background=(0, 0, 0)):
        """A ring of `slots` (2..8) pinned frames for deliver() / acquire() / release().  `format`: "rgba8", or 4:2:0 Y'CbCr for a
        video encoder, "nv12" / "i420" (BT.709; `full_range`: 0..255 instead of 16..235 / 16..240; `background`: the (R, G, B) the
        premultiplied frame is laid over, Y'CbCr having no alpha).  A Y'CbCr ring is opened only when none is open.
        delivery_set_overlay() then makes the ring deliver the selection overlay in place of the frame."""
        if format not in DELIVERY_FORMATS:
            raise ValueError("format must be one of %s" % ", ".join(sorted(DELIVERY_FORMATS)))
        self._slot_views = {}
        if format == "rgba8":
            self._check(self._L.gsr_delivery_open(self._ctx, slots))
            self._depth_ring = False
            return
        self._check(self._L.gsr_delivery_open_ex(self._ctx, ctypes.byref(self._delivery_options(slots, format, full_range, background))))
        self._depth_ring = False

    @staticmethod
    def _delivery_options(slots, format, full_range, background):
        bg = [int(v) for v in background]
        if len(bg) != 3 or min(bg) < 0 or max(bg) > 255:
            raise ValueError("background must be three bytes (R, G, B)")
        return GsrDeliveryOptions(slots, DELIVERY_FORMATS[format], 1 if full_range else 0, (ctypes.c_uint8 * 4)(*bg, 0))

    def open_delivery_depth(self, slots=3, format="rgba8", full_range=False, background=(0, 0, 0), depth="u16", depth_step=1, depth_near=0.1):
        """open_delivery's ring with a depth plane beside every frame (gsr_delivery_open_depth; opened only when no ring is open):
        colour exactly as open_delivery(slots, format, full_range, background) delivers it, and the frame's hit plane (read_depth()[1])
        sampled at every `depth_step`-th pixel (1 or 2) in both directions -- `depth` "f32": as it is; "u16": 16-bit inverse depth
        against `depth_near` (0: no hit, 65535: at or in front of depth_near; z ~ depth_near * 65535 / u).  acquire() then returns
        (serial, pixels or planes, depth).  depth=None: open_delivery.  (A method of its own, as the C ABI has an entry point of its
        own: open_delivery keeps the signature its callers know.)"""
        if format not in DELIVERY_FORMATS:
            raise ValueError("format must be one of %s" % ", ".join(sorted(DELIVERY_FORMATS)))
        if depth is None:
            return self.open_delivery(slots, format, full_range, background)
        if depth not in DEPTH_DELIVERY_FORMATS:
            raise ValueError("depth must be None or one of %s" % ", ".join(sorted(DEPTH_DELIVERY_FORMATS)))
        self._slot_views = {}
        opt = self._delivery_options(slots, format, full_range, background)
        dopt = GsrDepthDeliveryOptions(DEPTH_DELIVERY_FORMATS[depth], int(depth_step), float(depth_near), 0)
        self._check(self._L.gsr_delivery_open_depth(self._ctx, ctypes.byref(opt), ctypes.byref(dopt)))
        self._depth_ring = True

    def depth_layout(self):
        """The depth plane of the open depth ring's frames at the current size (gsr_delivery_depth_layout): format ("f32" / "u16"),
        step, width and height (Wd, Hd), stride, offset (bytes from the slot's first pixel), bytes, near."""
        lay = GsrDepthLayout()
        self._check(self._L.gsr_delivery_depth_layout(self._ctx, ctypes.byref(lay)))
        names = {v: k for k, v in DEPTH_DELIVERY_FORMATS.items()}
        return {"format": names[lay.format], "step": lay.step, "width": lay.width, "height": lay.height, "stride": lay.stride,
                "offset": int(lay.offset), "bytes": int(lay.bytes), "near": float(lay.near)}

    def delivery_layout(self):
        """The open ring's frame layout at the current size (gsr_delivery_layout): format, width, height, bytes (the payload) and
        planes, a list of {offset, stride, rows} -- one for RGBA8, Y and CbCr for NV12, Y, Cb and Cr for I420."""
        lay = GsrFrameLayout()
        self._check(self._L.gsr_delivery_layout(self._ctx, ctypes.byref(lay)))
        names = {v: k for k, v in DELIVERY_FORMATS.items()}
        return {"format": names[lay.format], "width": lay.width, "height": lay.height, "bytes": int(lay.bytes),
                "planes": [{"offset": int(lay.offset[k]), "stride": lay.stride[k], "rows": lay.rows[k]} for k in range(lay.planes)]}

    def close_delivery(self):
        self._slot_views = {}
        self._check(self._L.gsr_delivery_close(self._ctx))
        self._depth_ring = False

    def deliver(self):
        """Enqueue the delivery of the frame enqueued last (in a group: of the frame gathered last); returns its serial.
        No host wait.  Raises GsplatError with code GSR_ERR_BUSY, and enqueues nothing, when every slot is taken."""
        k = ctypes.c_uint64(0)
        self._check(self._L.gsr_deliver_frame_async(self._ctx, ctypes.byref(k)))
        return k.value

    def frame_ready(self, serial=0):
        rc = self._L.gsr_frame_ready(self._ctx, serial)
        if rc < 0:
            self._check(rc)
        return bool(rc)

    def acquire(self, serial=0):
        """Wait for frame `serial`'s copy (0: the oldest frame not acquired yet) -- not for the frames behind it -- and
        return (serial, pixels): a read-only zero-copy [H, W, 4] uint8 view of the slot's pinned block, valid until
        release(serial).  On a Y'CbCr ring: (serial, planes), a tuple of such views -- Y [H, W] and CbCr [Hc, Wc, 2] for "nv12",
        Y [H, W], Cb [Hc, Wc] and Cr [Hc, Wc] for "i420" (Hc = (H + 1) // 2, Wc = (W + 1) // 2), contiguous in the block: the
        payload a rawvideo pipe takes is the planes' bytes one after the other.  A frame that was not composited (list overflow) raises GsplatError with code GSR_ERR_OVERFLOW
        and frees its slot: render and deliver that pose again.
        On a depth ring (open_delivery_depth): (serial, pixels or planes, depth), depth a read-only zero-copy [Hd, Wd] float32 /
        uint16 view of the same block: the hit plane of the SAME frame (depth_layout())."""
        f = GsrFrame()
        self._check(self._L.gsr_acquire_frame(self._ctx, serial, ctypes.byref(f)))
        view = self._slot_views.get(f.slot)
        if view is None:
            lay = GsrFrameLayout()
            self._check(self._L.gsr_delivery_layout(self._ctx, ctypes.byref(lay)))
            block = np.frombuffer((ctypes.c_uint8 * lay.bytes).from_address(f.pixels), dtype=np.uint8)
            block.flags.writeable = False
            if lay.format == GSR_FORMAT_RGBA8:
                view = block.reshape(f.height, f.width, 4)
            else:   # Y [H, W]; NV12: CbCr [Hc, Wc, 2]; I420: Cb [Hc, Wc], Cr [Hc, Wc]
                planes = [block[lay.offset[k]:lay.offset[k] + lay.stride[k] * lay.rows[k]].reshape(lay.rows[k], lay.stride[k]) for k in range(lay.planes)]
                if lay.format == GSR_FORMAT_NV12:
                    planes[1] = planes[1].reshape(lay.rows[1], lay.stride[1] // 2, 2)
                view = tuple(planes)
            if self._depth_ring:
                dl = GsrDepthLayout()
                self._check(self._L.gsr_delivery_depth_layout(self._ctx, ctypes.byref(dl)))
                dtype = np.float32 if dl.format == GSR_DEPTH_F32 else np.uint16
                depth = np.frombuffer((ctypes.c_uint8 * dl.bytes).from_address(f.pixels + dl.offset), dtype=dtype).reshape(dl.height, dl.width)
                depth.flags.writeable = False
                view = (view, depth)
            self._slot_views[f.slot] = view
        if self._depth_ring:
            return f.serial, view[0], view[1]
        return f.serial, view

    def release(self, serial):
        self._check(self._L.gsr_release_frame(self._ctx, serial))

    # -- depth planes and picking (gsr_depth_async / gsr_read_depth / gsr_pick) --
    def set_hit_alpha(self, a):
        """Accumulated alpha at which a pixel's hit is taken, in (0, 1]; default 0.5."""
        self._check(self._L.gsr_set_hit_alpha(self._ctx, float(a)))

    def depth_async(self):
        """Enqueue the depth pass behind the frame enqueued last (no host wait)."""
        self._check(self._L.gsr_depth_async(self._ctx))

    def read_depth(self):
        """(mean, hit, index) of the last rendered frame, [H, W] each, row 0 = top.  Per pixel, over the fragments of its
        bin's list front to back (those the compositor's coverage test keeps, with the compositor's weight B), from T = 1,
        D = 0: w = T * B; D = fma(w, z, D); T -= w, z being the w of the splat centre's clip position.
        mean (float32): D, premultiplied like the colour channels (divide by the framebuffer's alpha for expected depth);
        hit (float32): z of the first fragment at which 1 - T reaches hit_alpha, +inf when none does;
        index (uint32): that fragment's splat index, 0xffffffff when none.
        Waits for the frame (one that did not fit its lists is rendered again first) and runs the pass if needed."""
        shape = (self.height, self.width)
        mean, hit, index = np.empty(shape, np.float32), np.empty(shape, np.float32), np.empty(shape, np.uint32)
        self._check(self._L.gsr_read_depth(self._ctx, mean.ctypes.data, hit.ctypes.data, index.ctypes.data))
        return mean, hit, index

    def pick(self, points):
        """The splat under each pixel of `points` ([(x, y), ...], at most 4096) in the last rendered frame: a structured
        array with index (uint32, 0xffffffff: none), depth (the hit's z, +inf: none), mean and alpha (= 1 - T) -- the same
        bits as read_depth() holds for those pixels."""
        xy = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 2)
        out = np.zeros(max(len(xy), 1), dtype=PICK_DTYPE)
        self._check(self._L.gsr_pick(self._ctx, xy.ctypes.data, len(xy), out.ctypes.data))
        return out[:len(xy)]

    # -- selection (gsr_select_* / gsr_selection_* / gsr_scene_erase_selected): one bit per splat, held with the device scene --
    @staticmethod
    def _select_code(table, name, what):
        if isinstance(name, str):
            if name not in table:
                raise ValueError("%s must be one of %s" % (what, ", ".join(sorted(table))))
            return table[name]
        return int(name)   # (a raw code: the library judges it)

    def select_region(self, rect, mask=None, mode="centre", op="replace"):
        """Pick splats by a screen region of the last rendered frame and fold them into the selection; returns the selected count.
        rect = (x0, y0, x1, y1): the pixels [x0, x1) x [y0, y1).  mask: optional [y1 - y0, stride] array (stride >= x1 - x0), non-zero =
        inside (a rasterised lasso or brush; row 0 is y0).  mode "centre": the listed splats whose centre pixel lies in the region
        ("select through"); "hit": the splats that are the hit of one or more of its pixels (read_depth()[2]; "select the
        surface").  op: "replace", "add", "subtract", "intersect"."""
        x0, y0, x1, y1 = (int(v) for v in rect)
        reg = GsrRegion(x0, y0, x1, y1, None, 0, 0)
        if mask is not None:
            m = np.ascontiguousarray(mask)
            if m.dtype != np.uint8:
                m = (m != 0).astype(np.uint8)
            if m.ndim != 2 or m.shape[0] < y1 - y0:
                raise ValueError("mask must be [y1 - y0, stride]")
            reg.mask, reg.mask_stride = m.ctypes.data, m.shape[1]
        count = ctypes.c_uint32(0)
        self._check(self._L.gsr_select_region(self._ctx, ctypes.byref(reg), self._select_code(SELECT_MODES, mode, "mode"),
                                              self._select_code(SELECT_OPS, op, "op"), ctypes.byref(count)))
        return count.value

    def select_box(self, box, op="replace"):
        """Pick the splats inside box = (xMin, xMax, yMin, yMax, zMin, zMax) -- scene_limit_box's comparisons; needs no frame."""
        box = np.ascontiguousarray(box, dtype=np.float64)
        count = ctypes.c_uint32(0)
        self._check(self._L.gsr_select_box(self._ctx, box.ctypes.data, self._select_code(SELECT_OPS, op, "op"), ctypes.byref(count)))
        return count.value

    def set_selection(self, picked=None, op="replace", words=None):
        """Fold a set of the host's into the selection: `picked` bool[n] (None: the empty set), or `words` uint32[>= ceil(n / 32)] as
        selection_words() returns them (bits at and above n are dropped)."""
        count = ctypes.c_uint32(0)
        code = self._select_code(SELECT_OPS, op, "op")
        if words is None and picked is not None:
            b = np.ascontiguousarray(picked).reshape(-1) != 0
            if b.size != self._count():
                raise ValueError("picked must hold one entry per splat (%d)" % self._count())
            words = pack_selection(b)
        if words is None:
            self._check(self._L.gsr_selection_set(self._ctx, None, 0, code, ctypes.byref(count)))
        else:
            w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
            self._check(self._L.gsr_selection_set(self._ctx, w.ctypes.data, w.size, code, ctypes.byref(count)))
        return count.value

    def invert_selection(self):
        count = ctypes.c_uint32(0)
        self._check(self._L.gsr_selection_invert(self._ctx, ctypes.byref(count)))
        return count.value

    def selection_words(self):
        """The selection as the device holds it: uint32[ceil(n / 32)], splat i = bit i & 31 of word i >> 5."""
        n = self._count()
        w = np.zeros(-(-n // 32), dtype=np.uint32)
        self._check(self._L.gsr_read_selection(self._ctx, w.ctypes.data if w.size else None, w.size, None))
        return w

    def selection_count(self):
        count = ctypes.c_uint32(0)
        self._check(self._L.gsr_read_selection(self._ctx, None, 0, ctypes.byref(count)))
        return count.value

    def selection(self):
        """bool[n]: which splats are selected."""
        return unpack_selection(self.selection_words(), self._count())

    def scene_erase_selected(self, keep=False):
        """Remove the selected splats (keep=True: the unselected ones) as scene_limit_box removes those outside its box; returns the new
        count.  When nothing would be removed nothing changes and the last frame stays valid."""
        n = ctypes.c_uint32(0)
        self._check(self._L.gsr_scene_erase_selected(self._ctx, 1 if keep else 0, ctypes.byref(n)))
        self._n = n.value
        return n.value

    # -- hidden splats (gsr_hide_selected / gsr_hidden_set / gsr_read_hidden / gsr_select_hidden): hide without erasing, show again --
    def hide_selected(self, op="add"):
        """Fold the selection into the hidden set: H = H op S -- "add" hides the selected splats, "subtract" shows them, "replace"
        hides exactly them, "intersect" keeps hidden only what is also selected; returns the hidden count.  A hidden splat is in no
        list of the frames rendered from now on (not drawn, not picked, no depth, no contribution); nothing is erased.  A scene
        edit like scene_translate: the next pick / select_region / read_depth needs a new frame."""
        count = ctypes.c_uint32(0)
        self._check(self._L.gsr_hide_selected(self._ctx, self._select_code(SELECT_OPS, op, "op"), ctypes.byref(count)))
        return count.value

    def set_hidden(self, hidden=None, op="replace", words=None):
        """Fold a set of the host's into the hidden set: `hidden` bool[n] (None: the empty set, so set_hidden(None) shows
        everything), or uint32 words as hidden_words() returns them (`words=`, or a uint32 array; bits at and above n are dropped)."""
        count = ctypes.c_uint32(0)
        code = self._select_code(SELECT_OPS, op, "op")
        if words is None and hidden is not None:
            a = np.ascontiguousarray(hidden)
            if a.dtype == np.uint32:
                words = a
            else:
                b = a.reshape(-1) != 0
                if b.size != self._count():
                    raise ValueError("hidden must hold one entry per splat (%d)" % self._count())
                words = pack_selection(b)
        if words is None:
            self._check(self._L.gsr_hidden_set(self._ctx, None, 0, code, ctypes.byref(count)))
        else:
            w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
            self._check(self._L.gsr_hidden_set(self._ctx, w.ctypes.data, w.size, code, ctypes.byref(count)))
        return count.value

    def hidden_words(self):
        """The hidden set as the device holds it: uint32[ceil(n / 32)], splat i = bit i & 31 of word i >> 5."""
        n = self._count()
        w = np.zeros(-(-n // 32), dtype=np.uint32)
        self._check(self._L.gsr_read_hidden(self._ctx, w.ctypes.data if w.size else None, w.size, None))
        return w

    def hidden_count(self):
        count = ctypes.c_uint32(0)
        self._check(self._L.gsr_read_hidden(self._ctx, None, 0, ctypes.byref(count)))
        return count.value

    def hidden(self):
        """bool[n]: which splats are hidden."""
        return unpack_selection(self.hidden_words(), self._count())

    def select_hidden(self, op="replace"):
        """Fold the hidden set into the selection (S = S op H), a picker like select_box; returns the selected count.
        select_hidden() + scene_erase_selected() erases the hidden splats for good."""
        count = ctypes.c_uint32(0)
        self._check(self._L.gsr_select_hidden(self._ctx, self._select_code(SELECT_OPS, op, "op"), ctypes.byref(count)))
        return count.value

    # -- editing the selection (gsr_selection_bounds / gsr_scene_*_selected): the selected splats and nothing else --
    def selection_bounds(self):
        """(count, min f32[3], max f32[3]): the selected splats and the axis-aligned box of their centres, reduced on the device.
        Nothing selected: (0, +inf, -inf); a NaN coordinate is counted and never enters the box."""
        b = GsrSelectionBounds()
        self._check(self._L.gsr_selection_bounds(self._ctx, ctypes.byref(b)))
        return int(b.count), np.array(b.min, dtype=np.float32), np.array(b.max, dtype=np.float32)

    @staticmethod
    def _pivot(pivot):
        return None if pivot is None else np.ascontiguousarray(pivot, dtype=np.float64).reshape(3)

    def scene_translate_selected(self, t):
        """scene_translate on the selected splats only: what Scene.translate would leave in a Scene holding only them.  A scene edit:
        the next pick / select_region / overlay needs a new frame; selection, hidden set and contribution state stay."""
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        self._check(self._L.gsr_scene_translate_selected(self._ctx, t.ctypes.data))

    def scene_rotate_selected(self, q_xyzw, pivot=None):
        """scene_rotate on the selected splats only; pivot (x, y, z): translate(-pivot), rotate, translate(+pivot), each step rounded
        to f32.  None is the rotation alone (not a pivot of zero).  Refused while set_sh_follow is on and the scene has SH rows."""
        q = np.ascontiguousarray(q_xyzw, dtype=np.float64).reshape(4)
        p = self._pivot(pivot)
        self._check(self._L.gsr_scene_rotate_selected(self._ctx, q.ctypes.data, None if p is None else p.ctypes.data))

    # -- rotating SH coefficients (gsr_scene_rotate_sh / _rotate_selected_sh / _bake_sh_frame) --
    def scene_rotate_sh(self, q_xyzw, selected=False):
        """Rotate, in place, the SH coefficients of every SH row (or of the selected splats' rows) by q = (x, y, z, w); returns the
        rows rotated.  Acts in the coefficients' own frame: the SH frame is neither read nor written.  A scene edit."""
        q = np.ascontiguousarray(q_xyzw, dtype=np.float64).reshape(4)
        rows = ctypes.c_uint32(0)
        self._check(self._L.gsr_scene_rotate_sh(self._ctx, q.ctypes.data, GSR_SH_SELECTED if selected else GSR_SH_ALL, ctypes.byref(rows)))
        return rows.value

    def scene_rotate_selected_sh(self, q_xyzw, pivot=None):
        """scene_rotate_selected and the selected splats' SH coefficients with it, as one edit.  Allowed with set_sh_follow on or
        off while the SH frame is the identity (scene_bake_sh_frame makes it one); without SH rows it is scene_rotate_selected."""
        q = np.ascontiguousarray(q_xyzw, dtype=np.float64).reshape(4)
        p = self._pivot(pivot)
        self._check(self._L.gsr_scene_rotate_selected_sh(self._ctx, q.ctypes.data, None if p is None else p.ctypes.data))

    def scene_bake_sh_frame(self):
        """Move an SH frame that is a rotation times a positive uniform scale into the coefficients; the frame becomes the identity.
        Returns the quaternion (x, y, z, w) float64[4] the coefficients were rotated by ((0, 0, 0, 1) for an identity frame)."""
        q = np.zeros(4, dtype=np.float64)
        self._check(self._L.gsr_scene_bake_sh_frame(self._ctx, q.ctypes.data))
        return q

    def scene_scale_selected(self, s, pivot=None):
        """scene_scale on the selected splats only; pivot as in scene_rotate_selected.  Components must be finite; 0 is allowed."""
        s = np.ascontiguousarray(s, dtype=np.float64).reshape(3)
        p = self._pivot(pivot)
        self._check(self._L.gsr_scene_scale_selected(self._ctx, s.ctypes.data, None if p is None else p.ctypes.data))

    def scene_set_rgba_selected(self, rgba, channels="rgba"):
        """Paint the selected splats: rgba = (r, g, b, a) bytes or the packed word r | g << 8 | b << 16 | a << 24; channels: which of
        "r", "g", "b", "a" are written (or a raw byte mask).  SH-coloured splats show only the opacity byte."""
        if isinstance(channels, str):
            if not channels or set(channels) - set("rgba"):
                raise ValueError('channels must be made of "r", "g", "b", "a"')
            mask = sum(0xff << (8 * "rgba".index(ch)) for ch in set(channels))
        else:
            mask = int(channels) & 0xffffffff
        if np.ndim(rgba):
            r, g, b, a = (int(v) & 0xff for v in rgba)
            rgba = r | g << 8 | b << 16 | a << 24
        self._check(self._L.gsr_scene_set_rgba_selected(self._ctx, int(rgba) & 0xffffffff, mask))

    # -- growing the scene (gsr_scene_reserve / _capacity / _duplicate_selected / _append_selected / _append_arrays) --
    def scene_reserve(self, rows):
        """Make the device scene's arrays hold at least `rows` splats, so that duplicates and appends up to that count re-allocate
        nothing and copy no old row.  Never shrinks; changes no splat and no frame state."""
        self._check(self._L.gsr_scene_reserve(self._ctx, int(rows)))

    def scene_capacity(self):
        """Rows the device scene's arrays hold (at least scene_count())."""
        rows = ctypes.c_uint32(0)
        self._check(self._L.gsr_scene_capacity(self._ctx, ctypes.byref(rows)))
        return rows.value

    def scene_duplicate_selected(self):
        """Copy the selected splats, in order and bit for bit, behind the scene's last splat; returns (first, count): the copies
        are the splats [first, first + count) and become the selection, so scene_translate_selected moves them next.  Existing
        indices, the hidden set and the contribution accumulators stay.  Nothing selected: (n, 0), nothing touched."""
        first, count = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(self._L.gsr_scene_duplicate_selected(self._ctx, ctypes.byref(first), ctypes.byref(count)))
        self._n = first.value + count.value
        return first.value, count.value

    def scene_append_selected(self, other):
        """scene_duplicate_selected with the rows read from `other`'s device scene and its selection (same GPU, device to device;
        `other` is not changed and its SH rows are not carried); returns (first, count)."""
        first, count = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(self._L.gsr_scene_append_selected(self._ctx, other._ctx, ctypes.byref(first), ctypes.byref(count)))
        self._n = first.value + count.value
        return first.value, count.value

    def scene_append_arrays(self, data, positions, rotations, scales):
        """Append rows given as set_scene_arrays takes them (the same repack and check); returns the index of the first new
        splat.  The new rows become the selection."""
        data = np.ascontiguousarray(data, dtype=np.uint32).reshape(-1)
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1)
        rot = np.ascontiguousarray(rotations, dtype=np.float32).reshape(-1)
        scl = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
        m = pos.size // 3
        if data.size < 8 * m or rot.size != 4 * m or scl.size != 3 * m:
            raise ValueError("data / rotations / scales do not hold %d splats" % m)
        first = ctypes.c_uint32(0)
        self._check(self._L.gsr_scene_append_arrays(self._ctx, data.ctypes.data, pos.ctypes.data, rot.ctypes.data, scl.ctypes.data, m, ctypes.byref(first)))
        self._n = first.value + m
        self._scene = None if m else self._scene
        return first.value

    # -- contribution (gsr_contrib_* / gsr_read_contrib / gsr_select_contrib): per-splat weight, peak and pixel counts over views --
    def contrib_reset(self):
        """Zero the scene's contribution accumulators and the pass counter (allocates them on first use); blocking."""
        self._check(self._L.gsr_contrib_reset(self._ctx))

    def contrib_accumulate(self):
        """Enqueue the contribution pass behind the frame enqueued last (no host wait): every fragment's weight w = T * B of that
        frame is added to its splat's accumulators.  A frame whose lists did not fit adds nothing and is not counted."""
        self._check(self._L.gsr_contrib_accumulate_async(self._ctx))

    def read_contrib(self):
        """(weight, peak, pixels, frames) accumulated since the last reset, one entry per splat.  weight (uint64): the sum over the
        splat's fragments of rint(w * 2^24), i.e. weight * 2^-24 is "fully opaque pixels' worth"; peak (float32): the largest w;
        pixels (uint32): the fragments (pixels the splat covered, whatever the weight; modulo 2^32); frames: the passes counted."""
        n = self._count()
        weight, peak, pixels = np.zeros(n, np.uint64), np.zeros(n, np.float32), np.zeros(n, np.uint32)
        frames = ctypes.c_uint32(0)
        self._check(self._L.gsr_read_contrib(self._ctx, weight.ctypes.data if n else None, peak.ctypes.data if n else None,
                                             pixels.ctypes.data if n else None, n, ctypes.byref(frames)))
        return weight, peak, pixels, frames.value

    def select_contrib(self, stat="weight", below=0.0, op="replace"):
        """Pick the splats whose accumulated value is below `below` (compared in f64 over ALL splats of the scene; one no frame
        ever listed has value 0) and fold them into the selection; returns the selected count.  stat: "weight" (weight * 2^-24),
        "peak" or "pixels".  Refused while no pass has contributed."""
        count = ctypes.c_uint32(0)
        self._check(self._L.gsr_select_contrib(self._ctx, self._select_code(CONTRIB_STATS, stat, "stat"), float(below),
                                               self._select_code(SELECT_OPS, op, "op"), ctypes.byref(count)))
        return count.value

    # -- splat data (gsr_attr_stats / gsr_attr_histogram / gsr_select_attr): an attribute's distribution, and a range of it as a picker --
    @staticmethod
    def _origin(origin):
        return None if origin is None else np.ascontiguousarray(origin, dtype=np.float64).reshape(3)

    @staticmethod
    def _scope(selected, visible):
        return (SCOPES["selected"] if selected else 0) | (SCOPES["visible"] if visible else 0)

    def attr_stats(self, attr, origin=None, selected=False, visible=False):
        """(count, nan, min, max) of an attribute (ATTRS: "opacity", "scale_max", "distance", ...) over the splats in scope --
        selected=True: only the selection; visible=True: only what is not hidden.  nan: values that are NaN; min / max over the
        others (+inf, -inf when there are none).  origin (x, y, z): what "distance" is measured from."""
        o = self._origin(origin)
        count, nan, mn, mx = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._L.gsr_attr_stats(self._ctx, self._select_code(ATTRS, attr, "attr"), None if o is None else o.ctypes.data,
                                           self._scope(selected, visible), ctypes.byref(count), ctypes.byref(nan), ctypes.byref(mn), ctypes.byref(mx)))
        return count.value, nan.value, mn.value, mx.value

    def attr_histogram(self, attr, lo, hi, bins, origin=None, selected=False, visible=False):
        """(counts uint32[bins], (below, above, nan), edges float64[bins + 1]): the attribute's values in [lo, hi) binned by the
        header's edge rule (attr_edges), and the splats in scope below lo, at or above hi, and NaN.
        select_attr(attr, edges[a], edges[b]) selects exactly counts[a:b].sum() splats of an unscoped histogram."""
        bins = int(bins)
        if not 1 <= bins <= ATTR_MAX_BINS:
            raise ValueError("bins must be in 1 .. %d" % ATTR_MAX_BINS)
        o = self._origin(origin)
        counts, outside = np.zeros(bins, np.uint32), np.zeros(3, np.uint32)
        self._check(self._L.gsr_attr_histogram(self._ctx, self._select_code(ATTRS, attr, "attr"), None if o is None else o.ctypes.data,
                                               self._scope(selected, visible), float(lo), float(hi), bins, counts.ctypes.data, outside.ctypes.data))
        return counts, (int(outside[0]), int(outside[1]), int(outside[2])), attr_edges(lo, hi, bins)

    def select_attr(self, attr, lo=-np.inf, hi=np.inf, origin=None, op="replace"):
        """Pick the splats with lo <= value < hi (all splats, hidden ones included; a NaN value is never picked) and fold them into
        the selection; returns the selected count."""
        o = self._origin(origin)
        count = ctypes.c_uint32(0)
        self._check(self._L.gsr_select_attr(self._ctx, self._select_code(ATTRS, attr, "attr"), None if o is None else o.ctypes.data,
                                            float(lo), float(hi), self._select_code(SELECT_OPS, op, "op"), ctypes.byref(count)))
        return count.value

    # -- neighbours (gsr_neighbours / gsr_select_neighbours): how many other splats lie within a radius of each; floaters have none --
    @staticmethod
    def _scope_flags(scope):
        names = (scope,) if isinstance(scope, str) else tuple(scope)
        for name in names:
            if name not in SCOPES:
                raise ValueError("unknown scope %r (one of %s)" % (name, ", ".join(SCOPES)))
        return sum(SCOPES[name] for name in set(names))

    @staticmethod
    def _neighbour_args(radius, cap, budget):
        cap = int(cap)
        if not 1 <= cap <= NEIGHBOUR_MAX_CAP:
            raise ValueError("cap must be in 1 .. %d" % NEIGHBOUR_MAX_CAP)
        budget = 0 if budget is None else int(budget)
        if budget < 0:
            raise ValueError("budget must not be negative")
        return float(radius), cap, budget

    def neighbours(self, radius, cap=64, scope=(), budget=None, counts=True, hist=True):
        """(counts uint32[n], hist uint32[cap + 1], info): for every splat in scope -- scope: any of "selected", "visible"; () is
        every splat -- the number of OTHER splats in scope within `radius` of it (f64, distance exactly radius counts), at most
        `cap`; 0 outside the scope.  hist[k]: the splats in scope with count == k, hist[cap] "cap or more"; hist.sum() ==
        info["in_scope"].  counts=False / hist=False: None in its place, nothing copied.  info: in_scope, nonfinite, pair_bound,
        budget.  budget=None is the library's default; a call whose pair_bound lies above it is refused (GsplatError) before
        the count pass runs, and the error carries `info`."""
        radius, cap, budget = self._neighbour_args(radius, cap, budget)
        n = self._count()
        c = np.zeros(n, np.uint32) if counts else None
        h = np.zeros(cap + 1, np.uint32) if hist else None
        info = GsrNeighbourInfo()
        self._check_neighbours(self._L.gsr_neighbours(self._ctx, radius, cap, self._scope_flags(scope), budget, c.ctypes.data if counts and n else None, n if counts else 0,
                                                      h.ctypes.data if hist else None, ctypes.byref(info)), info)
        return c, h, info.as_dict()

    def select_neighbours(self, radius, lo=0, hi=None, cap=64, scope=(), op="replace", budget=None):
        """(selected, info): pick the splats in scope with lo <= count < hi (hi=None: cap + 1, "lo or more") and fold them into the
        selection; counts as neighbours() gives them.  select_neighbours(r, hi=k) then scene_erase_selected() is the radius
        outlier filter: every splat with fewer than k neighbours within r goes.  With op "replace" it selects exactly
        hist[lo:hi].sum() splats of neighbours(radius, cap, scope)."""
        radius, cap, budget = self._neighbour_args(radius, cap, budget)
        hi = cap + 1 if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo <= hi <= cap + 1:
            raise ValueError("lo <= hi <= cap + 1 must hold")
        count, info = ctypes.c_uint32(0), GsrNeighbourInfo()
        self._check_neighbours(self._L.gsr_select_neighbours(self._ctx, radius, cap, self._scope_flags(scope), budget, lo, hi, self._select_code(SELECT_OPS, op, "op"),
                                                             ctypes.byref(count), ctypes.byref(info)), info)
        return count.value, info.as_dict()

    def _check_neighbours(self, rc, info):
        try:
            self._check(rc)
        except GsplatError as e:
            e.info = info.as_dict()   # (a call refused for its budget has filled it)
            raise

    # -- clusters (gsr_clusters / gsr_select_clusters / gsr_select_cluster_at): the connected islands of splats at a linking radius --
    @staticmethod
    def _cluster_args(radius, min_pts, budget):
        min_pts = int(min_pts)
        if not 0 <= min_pts <= NEIGHBOUR_MAX_CAP:
            raise ValueError("min_pts must be in 0 .. %d" % NEIGHBOUR_MAX_CAP)
        budget = 0 if budget is None else int(budget)
        if budget < 0:
            raise ValueError("budget must not be negative")
        return float(radius), min_pts, budget

    def clusters(self, radius, min_pts=0, scope=(), budget=None, labels=True, sizes=True):
        """(labels uint32[n], sizes uint32[n], info): the clusters of the splats in scope -- scope: any of "selected", "visible"; ()
        is every splat -- at the linking radius `radius` (f64, distance exactly radius links).  min_pts=0: connected components;
        min_pts=k: DBSCAN, a splat with k or more others within radius is core, core splats within radius of each other share a
        cluster, a non-core splat near a core one takes the smallest such label (border), the rest is noise.  labels[i]: the smallest
        splat index of i's cluster, CLUSTER_NONE for noise and outside the scope; sizes[i]: the splats labelled like i, 0 without a
        label.  labels=False / sizes=False: None in its place, nothing copied.  info: in_scope, nonfinite, pair_bound, budget, core,
        border, noise, clusters, largest_label, largest_size.  budget as neighbours() takes it: a call whose pair_bound lies above
        it is refused (GsplatError carrying `info`) before any walk runs."""
        radius, min_pts, budget = self._cluster_args(radius, min_pts, budget)
        n = self._count()
        lab = np.zeros(n, np.uint32) if labels else None
        siz = np.zeros(n, np.uint32) if sizes else None
        info = GsrClusterInfo()
        self._check_neighbours(self._L.gsr_clusters(self._ctx, radius, min_pts, self._scope_flags(scope), budget, lab.ctypes.data if labels and n else None,
                                                    siz.ctypes.data if sizes and n else None, n if labels or sizes else 0, ctypes.byref(info)), info)
        return lab, siz, info.as_dict()

    def select_clusters(self, radius, lo=0, hi=None, min_pts=0, scope=(), op="replace", budget=None):
        """(selected, info): pick the splats in scope whose cluster has lo <= size < hi splats (hi=None: no upper end; noise has
        size 0) and fold them into the selection.  select_clusters(r, hi=k) then scene_erase_selected() removes noise and every
        island smaller than k.  With op "replace" it selects exactly the splats in scope whose sizes[i] of clusters(radius,
        min_pts, scope) lies in the range."""
        radius, min_pts, budget = self._cluster_args(radius, min_pts, budget)
        hi = 0xffffffff if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo <= hi <= 0xffffffff:
            raise ValueError("0 <= lo <= hi < 2^32 must hold")
        count, info = ctypes.c_uint32(0), GsrClusterInfo()
        self._check_neighbours(self._L.gsr_select_clusters(self._ctx, radius, min_pts, self._scope_flags(scope), budget, lo, hi, self._select_code(SELECT_OPS, op, "op"),
                                                           ctypes.byref(count), ctypes.byref(info)), info)
        return count.value, info.as_dict()

    def select_cluster_at(self, radius, seed, min_pts=0, scope=(), op="replace", budget=None):
        """(selected, info): pick the cluster of splat `seed` -- an index, such as pick()'s, or "largest" for the largest cluster (ties:
        the smallest label) -- and fold it into the selection: the flood select.  A seed that is noise or outside the scope, or
        "largest" without a cluster, picks the empty set.  select_cluster_at(r, "largest"), invert_selection(),
        scene_erase_selected() keeps the largest island."""
        radius, min_pts, budget = self._cluster_args(radius, min_pts, budget)
        if isinstance(seed, str):
            if seed != "largest":
                raise ValueError("seed must be a splat index or \"largest\"")
            seed = CLUSTER_LARGEST
        else:
            seed = int(seed)
            if not 0 <= seed < CLUSTER_LARGEST:
                raise ValueError("seed must be a splat index or \"largest\"")
        count, info = ctypes.c_uint32(0), GsrClusterInfo()
        self._check_neighbours(self._L.gsr_select_cluster_at(self._ctx, radius, min_pts, self._scope_flags(scope), budget, seed, self._select_code(SELECT_OPS, op, "op"),
                                                             ctypes.byref(count), ctypes.byref(info)), info)
        return count.value, info.as_dict()

    # -- k nearest neighbours (gsr_knn / gsr_select_knn): per-splat neighbour lists, and statistical outlier removal --
    @staticmethod
    def _knn_args(radius, k, stat, budget):
        k = int(k)
        if not 1 <= k <= KNN_MAX_K:
            raise ValueError("k must be in 1 .. %d" % KNN_MAX_K)
        if stat not in KNN_STATS:
            raise ValueError("unknown stat %r (one of %s)" % (stat, ", ".join(KNN_STATS)))
        budget = 0 if budget is None else int(budget)
        if budget < 0:
            raise ValueError("budget must not be negative")
        return float(radius), k, KNN_STATS[stat], budget

    def knn(self, radius, k=8, stat="mean", scope=(), budget=None, found=True, idx=False, d2=False, values=True, hist=True):
        """(found uint32[n], idx uint32[n, k], d2 float64[n, k], values float64[n], hist uint32[k + 1], info): for every splat in
        scope -- scope: any of "selected", "visible"; () is every splat -- the k nearest OTHER splats in scope within `radius`,
        ascending by (squared distance, index): found[i] how many there are, idx / d2 their indices and squared distances, padded
        with KNN_NONE / +inf.  values[i]: stat "kth", the distance to the k-th (+inf without one); "mean", the mean distance to
        those found (+inf with none); NaN outside the scope.  hist[t]: the splats in scope with found == t.  A False argument:
        None in its place, nothing copied, and without idx and d2 the lists are not stored at all.  info: in_scope, nonfinite,
        pair_bound, budget, complete, finite_values, value_min, value_max.  budget as neighbours() takes it."""
        radius, k, stat, budget = self._knn_args(radius, k, stat, budget)
        n = self._count()
        f = np.zeros(n, np.uint32) if found else None
        i = np.full((n, k), KNN_NONE, np.uint32) if idx else None
        d = np.full((n, k), np.inf, np.float64) if d2 else None
        v = np.full(n, np.nan, np.float64) if values else None
        h = np.zeros(k + 1, np.uint32) if hist else None
        info = GsrKnnInfo()
        ptr = lambda a: a.ctypes.data if a is not None and n else None
        self._check_neighbours(self._L.gsr_knn(self._ctx, radius, k, self._scope_flags(scope), budget, stat, ptr(f), ptr(i), ptr(d), ptr(v),
                                               n if found or idx or d2 or values else 0, h.ctypes.data if hist else None, ctypes.byref(info)), info)
        return f, i, d, v, h, info.as_dict()

    def select_knn(self, radius, k=8, stat="mean", lo=0.0, hi=None, scope=(), op="replace", budget=None):
        """(selected, info): pick the splats in scope with lo <= value < hi (hi=None or +inf: no upper end, the +inf values
        included) and fold them into the selection; values as knn() gives them.  With op "replace" it selects exactly the
        splats in scope whose values[i] of knn(radius, k, stat, scope) satisfy the rule."""
        radius, k, stat, budget = self._knn_args(radius, k, stat, budget)
        lo, hi = float(lo), float("inf") if hi is None else float(hi)
        if lo != lo or hi != hi or lo > hi:
            raise ValueError("lo <= hi must hold, neither a NaN")
        count, info = ctypes.c_uint32(0), GsrKnnInfo()
        self._check_neighbours(self._L.gsr_select_knn(self._ctx, radius, k, self._scope_flags(scope), budget, stat, lo, hi, self._select_code(SELECT_OPS, op, "op"),
                                                      ctypes.byref(count), ctypes.byref(info)), info)
        return count.value, info.as_dict()

    def select_statistical_outliers(self, radius, k=8, std_ratio=2.0, scope=(), op="replace"):
        """(selected, threshold, info): statistical outlier removal.  The mean distance of every splat in scope to its k nearest
        within `radius` is read back; mu and the sample standard deviation sigma (n - 1) of the finite ones are taken in f64, and
        the splats with value >= threshold = mu + std_ratio * sigma -- those without a neighbour included -- are folded into the
        selection.  With fewer than two finite values only the splats without a neighbour are picked (threshold +inf).
        scene_erase_selected() then removes them."""
        values = self.knn(radius, k=k, stat="mean", scope=scope, found=False, hist=False)[3]
        threshold = knn_outlier_threshold(values, std_ratio)
        selected, info = self.select_knn(radius, k=k, stat="mean", lo=threshold, hi=None, scope=scope, op=op)
        return selected, threshold, info

    # -- normals (gsr_normals / gsr_select_normal): per-splat surface normals, selection by direction or surface variation --
    def _normal_options(self, radius, k, source, toward, scope, budget):
        if source not in NORMAL_SOURCES:
            raise ValueError("unknown source %r (one of %s)" % (source, ", ".join(NORMAL_SOURCES)))
        o = GsrNormalOptions()
        o.source = NORMAL_SOURCES[source]
        if source == "knn":
            if radius is None:
                raise ValueError("the knn source needs a radius")
            k = int(k)
            if not 2 <= k <= KNN_MAX_K:
                raise ValueError("k must be in 2 .. %d" % KNN_MAX_K)
            o.k, o.radius = k, float(radius)
        budget = 0 if budget is None else int(budget)
        if budget < 0:
            raise ValueError("budget must not be negative")
        o.scope, o.budget = self._scope_flags(scope), budget
        if toward is not None:
            o.oriented = 1
            o.toward[:] = [float(v) for v in np.asarray(toward, dtype=np.float64).reshape(3)]
        return o

    def normals(self, radius=None, k=8, source="knn", toward=None, scope=(), budget=None, normals=True, variation=True, found=True):
        """(normals float32[n, 3], variation float64[n], found uint32[n], info): a unit surface normal per splat in scope -- scope:
        any of "selected", "visible"; () is every splat.  source "knn": the eigenvector of the smallest eigenvalue of the covariance
        of the splat and its k nearest others in scope within `radius` (knn()'s lists; at least two are needed); "own": the
        splat's own shortest axis, no index and no walk.  variation[i] = l_min / (l_0 + l_1 + l_2): 0 on a plane, large at edges and
        corners.  toward=(x, y, z): every normal faces that viewpoint; None: its first non-zero component is positive.  A splat
        without a normal holds NaN in both; found[i] is the length of its list (0 for "own").  A False argument: None in its place,
        nothing copied.  info: in_scope, nonfinite, pair_bound, budget, valid, variation_min, variation_max.  budget as
        neighbours() takes it."""
        o = self._normal_options(radius, k, source, toward, scope, budget)
        n = self._count()
        nm = np.full((n, 3), np.nan, np.float32) if normals else None
        v = np.full(n, np.nan, np.float64) if variation else None
        f = np.zeros(n, np.uint32) if found else None
        info = GsrNormalInfo()
        ptr = lambda a: a.ctypes.data if a is not None and n else None
        self._check_neighbours(self._L.gsr_normals(self._ctx, ctypes.byref(o), ptr(nm), ptr(v), ptr(f), n if normals or variation or found else 0,
                                                   ctypes.byref(info)), info)
        return nm, v, f, info.as_dict()

    def select_normal(self, stat, lo=-np.inf, hi=np.inf, axis=None, radius=None, k=8, source="knn", toward=None, scope=(), op="replace", budget=None):
        """(selected, info): pick the splats with a normal whose value has lo <= value <= hi (both ends closed) and fold them into
        the selection.  stat "dot": n . axis; "abs_dot": |n . axis|, for normals that are not oriented -- select_normal("abs_dot",
        hi=0.2, axis=up, ..) is "the walls"; "variation": the surface variation, no axis.  The value is computed from the stored
        float32 normal, so with op "replace" exactly the splats that satisfy the rule on normals()' outputs for the same
        arguments are selected.  axis is used as given, not normalised."""
        if stat not in NORMAL_STATS:
            raise ValueError("unknown stat %r (one of %s)" % (stat, ", ".join(NORMAL_STATS)))
        o = self._normal_options(radius, k, source, toward, scope, budget)
        lo, hi = float(lo), float(hi)
        if lo != lo or hi != hi or lo > hi:
            raise ValueError("lo <= hi must hold, neither a NaN")
        a = None
        if stat != "variation":
            if axis is None:
                raise ValueError("stat %r needs an axis" % stat)
            a = np.ascontiguousarray(axis, dtype=np.float64).reshape(3)
        count, info = ctypes.c_uint32(0), GsrNormalInfo()
        self._check_neighbours(self._L.gsr_select_normal(self._ctx, ctypes.byref(o), NORMAL_STATS[stat], None if a is None else a.ctypes.data, lo, hi,
                                                         self._select_code(SELECT_OPS, op, "op"), ctypes.byref(count), ctypes.byref(info)), info)
        return count.value, info.as_dict()

    # -- merging cells (gsr_cells / gsr_scene_merge_cells): voxel simplification of the scene --
    @staticmethod
    def _cell_args(cell, cap, budget):
        cap = int(cap)
        if not 1 <= cap <= NEIGHBOUR_MAX_CAP:
            raise ValueError("cap must be in 1 .. %d" % NEIGHBOUR_MAX_CAP)
        budget = 0 if budget is None else int(budget)
        if budget < 0:
            raise ValueError("budget must not be negative")
        return float(cell), cap, budget

    def cells(self, cell, cap=64, scope=(), leaders=False, budget=None):
        """(leader uint32[n] or None, hist uint32[cap + 1], info): the report of scene_merge_cells(cell, scope).  The candidates
        -- the splats in scope (any of "selected", "visible"; () is every splat) whose position, rotation and scale are finite --
        fall into the cells of a grid of side `cell`; leader[i] (leaders=True) is the smallest candidate index of i's cell,
        CELL_NONE for a splat that is no candidate; hist[k] the cells with k members, hist[cap] "cap or more".  info: in_scope,
        candidates, cells, merged_cells, merged_members, largest, rows_after, pair_bound, budget.  budget as neighbours() takes it."""
        cell, cap, budget = self._cell_args(cell, cap, budget)
        n = self._count()
        lead = np.full(n, CELL_NONE, np.uint32) if leaders else None
        h = np.zeros(cap + 1, np.uint32)
        info = GsrCellInfo()
        self._check_neighbours(self._L.gsr_cells(self._ctx, cell, cap, self._scope_flags(scope), budget, lead.ctypes.data if leaders and n else None,
                                                 n if leaders else 0, h.ctypes.data, ctypes.byref(info)), info)
        return lead, h, info.as_dict()

    def scene_merge_cells(self, cell, scope=(), budget=None):
        """(new_count, info): every grid cell of side `cell` that holds two or more candidates becomes one splat, by moment matching
        -- the opacity x volume weighted mean, the covariance of the mixture, a rotation and scale from its eigen-decomposition --
        written at the smallest member's row; the other members are removed as scene_erase_selected() removes.  new_count equals
        cells(cell, scope=scope)[2]["rows_after"]; afterwards the selection is exactly the merged rows.  Nothing to merge: nothing
        changes.  A scene with SH rows is refused."""
        cell, _, budget = self._cell_args(cell, 1, budget)
        count, info = ctypes.c_uint32(0), GsrCellInfo()
        self._check_neighbours(self._L.gsr_scene_merge_cells(self._ctx, cell, self._scope_flags(scope), budget, ctypes.byref(count), ctypes.byref(info)), info)
        self._n = count.value
        return count.value, info.as_dict()

    # -- planes (gsr_fit_plane / gsr_plane_inliers / gsr_select_plane / gsr_plane_alignment): the floor found, selected by, aligned to --
    @staticmethod
    def _plane_args(threshold, count, budget, what):
        count = int(count)
        if not 1 <= count <= PLANE_MAX_HYPOTHESES:
            raise ValueError("%s must be in 1 .. %d" % (what, PLANE_MAX_HYPOTHESES))
        budget = 0 if budget is None else int(budget)
        if budget < 0:
            raise ValueError("budget must not be negative")
        return float(threshold), count, budget

    def fit_plane(self, threshold, hypotheses=512, seed=0, scope=(), budget=0, scores=False):
        """(plane, info[, scores]): the dominant plane of the splats in scope -- scope: any of "selected", "visible"; () is every
        splat -- by RANSAC on the device: `hypotheses` planes through three candidates each, drawn by a counter-based generator
        from `seed`, every one scored by the candidates within `threshold` of it (f64, a distance of exactly threshold counts);
        the largest score wins, ties go to the smallest index.  plane: float64[4] (nx, ny, nz, d), unit normal, or None when
        every hypothesis is degenerate.  info: in_scope, nonfinite, hypotheses, degenerate, found, best, triple, inliers, tests,
        budget, plane.  scores=True: also uint32[hypotheses].  A call whose tests = hypotheses * candidates lie above the budget
        (0: the library's default) is refused (GsplatError) before the scoring pass runs, and the error carries `info`."""
        threshold, hypotheses, budget = self._plane_args(threshold, hypotheses, budget, "hypotheses")
        sc = np.zeros(hypotheses, np.uint32) if scores else None
        info = GsrPlaneInfo()
        self._check_neighbours(self._L.gsr_fit_plane(self._ctx, threshold, hypotheses, int(seed) & 0xffffffffffffffff, self._scope_flags(scope), budget,
                                                     sc.ctypes.data if scores else None, ctypes.byref(info)), info)
        d = info.as_dict()
        plane = d["plane"].copy() if d["found"] else None
        return (plane, d, sc) if scores else (plane, d)

    def plane_inliers(self, planes, threshold, scope=(), budget=0, info=False):
        """uint32[K]: for each of the K planes (a, b, c, d) -- used as given, not normalised -- the splats in scope with a finite
        position within `threshold` of it: fit_plane's scoring pass alone.  info=True: (inliers, info)."""
        p = np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 4)
        threshold, count, budget = self._plane_args(threshold, p.shape[0], budget, "the number of planes")
        out = np.zeros(count, np.uint32)
        got = GsrPlaneInfo()
        self._check_neighbours(self._L.gsr_plane_inliers(self._ctx, p.ctypes.data, count, threshold, self._scope_flags(scope), budget, out.ctypes.data,
                                                         ctypes.byref(got)), got)
        return (out, got.as_dict()) if info else out

    def select_plane(self, plane, lo=-np.inf, hi=np.inf, within=None, op="replace"):
        """Pick the splats whose signed distance s from `plane` has lo <= s <= hi (all splats, hidden ones included; a NaN distance
        is never picked) and fold them into the selection; returns the selected count.  within=t is lo=-t, hi=t: after a fit over
        every splat, select_plane(plane, within=threshold) selects exactly info["inliers"] splats; select_plane(plane, hi=-t) is
        "everything under the floor"."""
        if within is not None:
            lo, hi = -float(within), float(within)
        p = np.ascontiguousarray(plane, dtype=np.float64).reshape(4)
        count = ctypes.c_uint32(0)
        self._check(self._L.gsr_select_plane(self._ctx, p.ctypes.data, float(lo), float(hi), self._select_code(SELECT_OPS, op, "op"), ctypes.byref(count)))
        return count.value

    @staticmethod
    def plane_alignment(plane, axis=(0, 1, 0)):
        """(q_xyzw float64[4], t float64[3]): the whole-scene rotation and translation that take `plane` to axis . p = 0 --
        scene_rotate(q) then scene_translate(t) puts the floor at y = 0.  A pure function of the library's: no device."""
        return plane_alignment(plane, axis)

    # -- matching and registration (gsr_match / gsr_select_match / gsr_register): this scene matched to another one, aligned with it --
    @staticmethod
    def _match_args(target, radius, budget):
        if not isinstance(target, HIPRenderer):
            raise TypeError("target must be a HIPRenderer")
        budget = 0 if budget is None else int(budget)
        if budget < 0:
            raise ValueError("budget must not be negative")
        return float(radius), budget

    def match(self, target, radius, transform=None, scope=(), target_scope=(), idx=True, d2=True, sums=False, budget=None):
        """(idx uint32[n], d2 float64[n], sums, info): for every splat of this scene in `scope`, moved by `transform` (3 x 4, R | t;
        None is the identity), the nearest splat of `target`'s scene in `target_scope` within `radius` -- smallest in (squared
        distance, index), f64, a distance of exactly radius counting.  Unmatched: MATCH_NONE and +inf; outside the scope: MATCH_NONE
        and NaN.  sums=True: {"pairs", "sum" float64[16]}, what rigid_solve takes -- the rows (T, Q, T_a * Q_b, d2) of the matched
        splats summed by a fixed tree; otherwise None.  idx=False / d2=False: None in its place, nothing copied.  info: in_scope,
        nonfinite, target_indexed, matched, pair_bound, budget, d2_min, d2_max.  budget as neighbours() takes it.  Neither scene
        is written; `target` may be this renderer."""
        radius, budget = self._match_args(target, radius, budget)
        m = _transform_arg(transform)
        n = self._count()
        i = np.full(n, MATCH_NONE, np.uint32) if idx else None
        d = np.full(n, np.nan, np.float64) if d2 else None
        s = GsrMatchSums() if sums else None
        info = GsrMatchInfo()
        ptr = lambda a: a.ctypes.data if a is not None and n else None
        self._check_neighbours(self._L.gsr_match(self._ctx, target._ctx, None if m is None else m.ctypes.data, radius, self._scope_flags(scope),
                                                 self._scope_flags(target_scope), budget, ptr(i), ptr(d), n if idx or d2 else 0,
                                                 ctypes.byref(s) if sums else None, ctypes.byref(info)), info)
        return i, d, s.as_dict() if sums else None, info.as_dict()

    def select_match(self, target, radius, lo=0.0, hi=None, transform=None, scope=(), target_scope=(), op="replace", budget=None):
        """(selected, info): pick the splats in scope whose distance v to their match has lo <= v < hi (hi=None or +inf: no upper end,
        the unmatched splats included) and fold them into the selection.  select_match(t, r, hi=r) is "what the other capture
        already has", select_match(t, r, lo=r) "what it lacks".  With op "replace" it selects exactly the splats whose d2 of
        match() with the same arguments satisfies the rule."""
        radius, budget = self._match_args(target, radius, budget)
        m = _transform_arg(transform)
        lo, hi = float(lo), float("inf") if hi is None else float(hi)
        if lo != lo or hi != hi or lo > hi:
            raise ValueError("lo <= hi must hold, neither a NaN")
        count, info = ctypes.c_uint32(0), GsrMatchInfo()
        self._check_neighbours(self._L.gsr_select_match(self._ctx, target._ctx, None if m is None else m.ctypes.data, radius, self._scope_flags(scope),
                                                        self._scope_flags(target_scope), budget, lo, hi, self._select_code(SELECT_OPS, op, "op"),
                                                        ctypes.byref(count), ctypes.byref(info)), info)
        return count.value, info.as_dict()

    def register(self, target, radius, transform=None, max_iterations=32, tolerance=2.0 ** -40, history=False, scope=(), target_scope=(), budget=None):
        """(M float64[3, 4], info): the rigid transform that takes this scene onto `target`'s, by iterating match, reduce and solve
        from `transform` (None: the identity) -- the same bits on every run.  It stops with status "too_few" when a step matches
        fewer than 3 splats, "converged" when a step's motion differs from the identity by at most `tolerance` in every entry,
        "max_iterations" after that many steps (1 .. 256).  info: status, iterations, pairs and rms of the last step, delta;
        history=True adds step_pairs and step_rms, one entry per step.  The scene is not written: rigid_decompose(M), then
        scene_rotate and scene_translate, apply the result once."""
        radius, budget = self._match_args(target, radius, budget)
        max_iterations = int(max_iterations)
        if not 1 <= max_iterations <= REGISTER_MAX_ITERATIONS:
            raise ValueError("max_iterations must be in 1 .. %d" % REGISTER_MAX_ITERATIONS)
        m = _transform_arg(transform)
        out = np.zeros(12, np.float64)
        info = GsrRegisterInfo()
        sp, sr = np.zeros(max_iterations, np.uint64), np.zeros(max_iterations, np.float64)
        if history:
            info.step_pairs, info.step_rms, info.step_rows = sp.ctypes.data, sr.ctypes.data, max_iterations
        self._check(self._L.gsr_register(self._ctx, target._ctx, None if m is None else m.ctypes.data, radius, self._scope_flags(scope),
                                         self._scope_flags(target_scope), budget, max_iterations, float(tolerance), out.ctypes.data, ctypes.byref(info)))
        d = info.as_dict()
        if history:
            d["step_pairs"], d["step_rms"] = sp[:info.iterations].copy(), sr[:info.iterations].copy()
        return out.reshape(3, 4), d

    # -- point-to-plane registration (gsr_match_surface / gsr_register_surface): aligned along the target's normals --
    def _surface_normals(self, target, normals, target_scope):
        """gsr_normal_options for the TARGET's normals: normals = dict(source="own" | "knn", radius=, k=, budget=); None is "own"."""
        nm = dict(normals or {})
        unknown = set(nm) - {"source", "radius", "k", "budget"}
        if unknown:
            raise ValueError("unknown normals option(s): %s" % ", ".join(sorted(unknown)))
        return target._normal_options(nm.get("radius"), nm.get("k", 8), nm.get("source", "own"), None, target_scope, nm.get("budget"))

    def match_surface(self, target, radius, normals=None, transform=None, scope=(), target_scope=(), budget=None):
        """(sums, info): one point-to-plane step as data.  The match is match()'s; sums = {"pairs", "surface_pairs", "sum"
        float64[29]}, what surface_solve takes -- per matched splat whose match has a normal the row (J_a * J_b for a <= b, J_a * r,
        r * r, d2) with J = (T x n, n) and r = n . (T - Q), summed by the fixed tree.  normals: how `target`'s normals are made,
        dict(source="own" | "knn", radius=, k=) as normals() takes them, over target_scope; None is "own".  info as match()'s.
        Neither scene is written; `target` may be this renderer."""
        radius, budget = self._match_args(target, radius, budget)
        o = self._surface_normals(target, normals, target_scope)
        m = _transform_arg(transform)
        s, info = GsrSurfaceSums(), GsrMatchInfo()
        self._check_neighbours(self._L.gsr_match_surface(self._ctx, target._ctx, None if m is None else m.ctypes.data, radius, self._scope_flags(scope),
                                                         self._scope_flags(target_scope), budget, ctypes.byref(o), ctypes.byref(s), ctypes.byref(info)), info)
        return s.as_dict(), info.as_dict()

    def register_surface(self, target, radius, normals=None, transform=None, max_iterations=32, tolerance=2.0 ** -40, history=False, scope=(), target_scope=(),
                         budget=None):
        """(M float64[3, 4], info): register()'s loop with point-to-plane steps -- every source point is pulled toward the target's
        SURFACE along the normal of its match, not toward the nearest sample, which converges in far fewer steps on floors, walls
        and table tops and does not stop at a biased pose.  The same bits on every run.  It stops with status "too_few" when a step
        has fewer than 6 pairs with a normal, "degenerate" when the residuals leave a direction free (a target of one or two
        planes), "converged" and "max_iterations" as register().  normals as match_surface() takes them; they are made once per
        call.  info: status, iterations, pairs, surface_pairs, rms, surface_rms and delta of the last step, valid (target splats
        with a normal); history=True adds step_pairs, step_surface_pairs, step_rms and step_surface_rms.  The scene is not written."""
        radius, budget = self._match_args(target, radius, budget)
        max_iterations = int(max_iterations)
        if not 1 <= max_iterations <= REGISTER_MAX_ITERATIONS:
            raise ValueError("max_iterations must be in 1 .. %d" % REGISTER_MAX_ITERATIONS)
        o = self._surface_normals(target, normals, target_scope)
        m = _transform_arg(transform)
        out = np.zeros(12, np.float64)
        info = GsrRegisterSurfaceInfo()
        steps = {"step_pairs": np.zeros(max_iterations, np.uint64), "step_surface_pairs": np.zeros(max_iterations, np.uint64),
                 "step_rms": np.zeros(max_iterations, np.float64), "step_surface_rms": np.zeros(max_iterations, np.float64)}
        if history:
            for k, a in steps.items():
                setattr(info, k, a.ctypes.data)
            info.step_rows = max_iterations
        self._check(self._L.gsr_register_surface(self._ctx, target._ctx, None if m is None else m.ctypes.data, radius, self._scope_flags(scope),
                                                 self._scope_flags(target_scope), budget, ctypes.byref(o), max_iterations, float(tolerance), out.ctypes.data,
                                                 ctypes.byref(info)))
        d = info.as_dict()
        if history:
            for k, a in steps.items():
                d[k] = a[:info.iterations].copy()
        return out.reshape(3, 4), d

    # -- selection overlay (gsr_set_overlay / gsr_overlay_async / gsr_read_overlay*): the selected splats tinted --
    def set_overlay(self, tint=(1.0, 0.5, 0.0), mix=0.5):
        """The overlay's options: selected splats are drawn with lerp(colour, tint, mix); tint (r, g, b) as the framebuffer's
        channels, mix in [0, 1].  tint=None: off, the overlay's buffers are freed."""
        if tint is None:
            self._check(self._L.gsr_set_overlay(self._ctx, None))
            return
        t = [float(v) for v in tint]
        if len(t) != 3:
            raise ValueError("tint must be three values (r, g, b)")
        opt = GsrOverlayOptions((ctypes.c_float * 3)(*t), float(mix), (ctypes.c_int32 * 4)())
        self._check(self._L.gsr_set_overlay(self._ctx, ctypes.byref(opt)))

    def set_overlay_outline(self, rgb=(1.0, 1.0, 1.0), alpha=1.0, threshold=0.5, width=2, side="outer"):
        """The selection's outline, drawn into the overlay image behind every pass (needs set_overlay): a pixel is inside where
        cover >= threshold; side "outer" draws the pixels around the selection within `width` (1 .. 16) of an inside pixel, "inner"
        the inside pixels within `width` of one that is not.  An edge pixel becomes lerp(overlay, rgb, alpha), its alpha
        lerp(a, 1, alpha).  rgb=None: off.  Everything that shows the overlay -- read_overlay*, a ring with delivery_set_overlay --
        shows the outline; cover does not change."""
        if rgb is None:
            self._check(self._L.gsr_set_overlay_outline(self._ctx, None))
            return
        t = [float(v) for v in rgb]
        if len(t) != 3:
            raise ValueError("rgb must be three values (r, g, b)")
        opt = GsrOutlineOptions((ctypes.c_float * 3)(*t), float(alpha), float(threshold), int(width),
                                self._select_code(OUTLINE_SIDES, side, "side"), (ctypes.c_int32 * 5)())
        self._check(self._L.gsr_set_overlay_outline(self._ctx, ctypes.byref(opt)))

    def overlay_async(self):
        """Enqueue the overlay pass behind the frame enqueued last (no host wait)."""
        self._check(self._L.gsr_overlay_async(self._ctx))

    def read_overlay(self):
        """(rgba, cover) of the last rendered frame: rgba float32 [H, W, 4], the frame with the selected splats tinted, premultiplied
        like readPixelsFloat(); cover float32 [H, W], the share of the pixel's alpha that selected splats supply.  Waits for the frame
        (one that did not fit its lists is rendered again first) and runs the pass if the image is not the one of this frame, this
        selection and these options."""
        rgba = np.empty((self.height, self.width, 4), np.float32)
        cover = np.empty((self.height, self.width), np.float32)
        self._check(self._L.gsr_read_overlay(self._ctx, rgba.ctypes.data, cover.ctypes.data))
        return rgba, cover

    def read_overlay_rgba8(self):
        """read_overlay()[0] as RGBA8 [H, W, 4], by the rule of readPixels()."""
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._L.gsr_read_overlay_rgba8(self._ctx, out.ctypes.data))
        return out

    def delivery_set_overlay(self, on=True):
        """The open ring (open_delivery / open_delivery_depth) delivers the selection overlay in place of the frame from now on
        (needs set_overlay; refused in a group); on=False: the frame again.  A newly opened ring starts with it off.  (A method
        of its own, as the C ABI has an entry point of its own: open_delivery keeps the signature its callers know.)"""
        self._check(self._L.gsr_delivery_set_overlay(self._ctx, 1 if on else 0))

    def read_keys(self):
        keys = np.empty(self._count(), dtype=np.uint32)
        mm = np.zeros(2, dtype=np.int32)
        self._check(self._L.gsr_read_keys(self._ctx, keys.ctypes.data, mm.ctypes.data))
        return keys, (int(mm[0]), int(mm[1]))

    def read_records(self):
        rec = np.empty((self._count(), 8), dtype=np.float32)
        bbox = np.empty((self._n, 4), dtype=np.int32)
        self._check(self._L.gsr_read_records(self._ctx, rec.ctypes.data, bbox.ctypes.data))
        return rec, bbox

    def stats(self):
        t = GsrTimings()
        self._check(self._L.gsr_get_timings(self._ctx, ctypes.byref(t)))
        return {k: getattr(t, k) for k, _ in GsrTimings._fields_}

    def reset_stats(self):
        self._check(self._L.gsr_reset_timings(self._ctx))

    def device_info(self):
        name = ctypes.create_string_buffer(256)
        cus, clk = ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._L.gsr_device_info(self._ctx, name, 256, ctypes.byref(cus), ctypes.byref(clk)))
        return {"name": name.value.decode(), "compute_units": cus.value, "clock_khz": clk.value}

    def bin_totals(self):
        """Entries per 32x32 bin of the last frame, shape [nby, nbx] (this context's band)."""
        nbx_all, nby_all = -(-self.width // 32), -(-self.height // 32)
        out = np.zeros(nbx_all * nby_all, dtype=np.uint32)
        nbx, nby = ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._L.gsr_read_bin_totals(self._ctx, out.ctypes.data, ctypes.byref(nbx), ctypes.byref(nby)))
        return out[:nbx.value * nby.value].reshape(nby.value, nbx.value)

    def bin_lists(self):
        """The last frame's bin lists: (starts [bins + 1], list [entries]) -- splat indices, front to back inside each 32x32 bin."""
        nbins = self.bin_totals().size
        starts = np.zeros(nbins + 1, dtype=np.uint32)
        self._check(self._L.gsr_read_bin_lists(self._ctx, starts.ctypes.data, None, 0))
        lst = np.zeros(max(int(starts[-1]), 1), dtype=np.uint32)
        self._check(self._L.gsr_read_bin_lists(self._ctx, starts.ctypes.data, lst.ctypes.data, lst.size))
        return starts, lst[:int(starts[-1])]

    def work_items(self):
        """How the last frame's bin lists were cut for the compositor: entries per segment, work items, the compositor's waves
        per 16x16 tile (which of its two kernels ran), bins.  ("speculative" is always False: the option is gone.)"""
        out = np.zeros(5, dtype=np.uint32)
        self._check(self._L.gsr_read_work_items(self._ctx, out.ctypes.data))
        return {"seg_len": int(out[0]), "items": int(out[1]), "speculative": bool(out[2]), "waves_per_tile": int(out[3]), "bins": int(out[4])}

    def work_list(self, max_items):
        """The last frame's compositor work list as k_bin_finalize published it (a test read-back, not part of the ABI):
        (items [n_items, 4] -- bin | segment << 16, first entry, end, the bin's first partial slot | its segments << 25 --,
        seg_start [bins + 1]).  `max_items`: the most items to expect (the compositor plan's max_items).  A frame whose lists
        did not fit is not rendered again: it has no items."""
        fn = self._L.gsr_debug_read_work_list
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
        items = np.zeros((max(int(max_items), 1), 4), dtype=np.uint32)
        seg_start = np.zeros(self.work_items()["bins"] + 1, dtype=np.uint32)
        n = fn(self._ctx, items.ctypes.data, items.size, seg_start.ctypes.data, seg_start.size)
        if n < 0:
            self._check(n)
        return items[:n].copy(), seg_start

    def frame_figures(self):
        """What the finalize step of the last frame saw and decided (a test read-back, not part of the ABI): the projection's
        four sums (visible splats, 16x16 tile overlaps, optical depth over the boxes, raw optical mass), the list entries, the
        longest list, the entries from which a bin is one work item, and the decisions."""
        fn = self._L.gsr_debug_read_frame_figures
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]
        w = np.zeros(8, dtype=np.uint64)
        self._check(fn(self._ctx, w.ctypes.data))
        out = {k: int(w[i]) for i, k in enumerate(("visible", "tiles", "otiles", "omass", "entries", "mxbin", "long_from"))}
        out.update({k: bool(int(w[7]) >> i & 1) for i, k in enumerate(("dense", "heavy", "by_size", "fits"))})
        return out

    def set_timing_interval(self, every):
        """Record stage events only on every `every`-th frame (they cost command-processor time on short frames)."""
        self._check(self._L.gsr_set_timing_interval(self._ctx, every))

    def convert_rgba8_async(self):
        self._check(self._L.gsr_convert_rgba8_async(self._ctx))

    def pack_band_rgba8_async(self, slab_ptr, slab_width_px):
        """This context's band as RGBA8 into the all-gather slab (device pointer), on the renderer's stream."""
        self._check(self._L.gsr_pack_band_rgba8_async(self._ctx, ctypes.c_void_p(slab_ptr), slab_width_px))

    def unpack_slabs_rgba8_async(self, gathered_ptr, image_ptr, slab_width_px, edges, stream_handle):
        """Gathered slabs [world][H][slab_w] -> row-major image, on `stream_handle` (the collective's stream).
        `edges`: [(x0, x1)] per rank, or the pair of ctypes arrays `edge_arrays(edges)` returns (per-frame callers)."""
        x0, x1 = edges if isinstance(edges, tuple) and not isinstance(edges[0], (tuple, list)) else edge_arrays(edges)
        self._check(self._L.gsr_unpack_slabs_rgba8_async(self._ctx, ctypes.c_void_p(gathered_ptr), ctypes.c_void_p(image_ptr),
                                                         slab_width_px, len(x0), x0, x1, ctypes.c_void_p(stream_handle)))

    def framebuffer8_ptr(self):
        return self._L.gsr_framebuffer8_device_ptr(self._ctx)

    def framebuffer_ptr(self):
        return self._L.gsr_framebuffer_device_ptr(self._ctx)

    def stream_order(self, other_stream_handle, ctx_waits):
        """Device-side ordering with another stream (see gsr_stream_order)."""
        self._check(self._L.gsr_stream_order(self._ctx, ctypes.c_void_p(other_stream_handle), 1 if ctx_waits else 0))

    def stream_handle(self):
        return self._L.gsr_stream_handle(self._ctx)

    # -- multi-GPU frame exchange inside the library (RCCL all-gather; see include/gsplat_hip.h) --
    def join_group(self, comm_id, rank, world, edges):
        """Collective: every rank calls it with the same 128-byte id (new_group_id() on rank 0, handed round by the
        host) and the same band edges [(x0, x1)] per rank.  Afterwards render_async() + allgather_frame_async()
        leave the whole RGBA8 frame on every rank (read_frame())."""
        cid = (ctypes.c_uint8 * GSR_COMM_ID_BYTES).from_buffer_copy(bytes(comm_id))
        x0, x1 = edge_arrays(edges)
        self._check(self._L.gsr_comm_init(self._ctx, cid, rank, world, x0, x1))

    def share_group(self, leader):
        """This context (another frame in flight of the same rank) uses `leader`'s communicator and exchange stream."""
        self._check(self._L.gsr_comm_share(self._ctx, leader._ctx))

    def join_group_custom(self, rank, world, edges, allgather):
        """Test hook (gsr_comm_init_custom): `allgather(send_ptr, recv_ptr, bytes_per_rank, stream)` replaces ncclAllGather."""
        x0, x1 = edge_arrays(edges)

        def _cb(user, send, recv, nbytes, stream):
            try:
                allgather(send, recv, int(nbytes), stream)
                return 0
            except Exception:      # never let an exception cross the C frame
                import traceback
                traceback.print_exc()
                return 1
        self._allgather_cb = ALLGATHER_FN(_cb)   # keep the trampoline alive as long as the context
        self._check(self._L.gsr_comm_init_custom(self._ctx, rank, world, x0, x1, self._allgather_cb, None))

    def leave_group(self):
        self._check(self._L.gsr_comm_destroy(self._ctx))

    def allgather_frame_async(self):
        self._check(self._L.gsr_allgather_frame_async(self._ctx))

    def read_frame(self):
        out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        self._check(self._L.gsr_read_frame_rgba8(self._ctx, out.ctypes.data))
        return out

    def frame8_ptr(self):
        return self._L.gsr_frame8_device_ptr(self._ctx)

    # -- depth in a group (gsr_comm_set_depth): the ranks exchange depth slabs beside the colour slabs --
    def set_group_depth(self, depth="u16", depth_step=1, near=0.1):
        """Opt this context, which has joined a group, into exchanging depth: every allgather_frame_async() then also leaves the
        frame's gathered hit plane on every rank -- read_frame_depth(), or the depth of acquire() on a ring opened with
        open_delivery_depth(depth=..., depth_step=..., depth_near=near) -- bit for bit the plane a depth ring with these options
        delivers on one context rendering the whole image.  `depth`: "u16", "f32", or None to switch it off again.  Every rank and
        every sharer passes the same options."""
        if depth is None:
            self._check(self._L.gsr_comm_set_depth(self._ctx, None))
            return
        if depth not in DEPTH_DELIVERY_FORMATS:
            raise ValueError("depth must be None or one of %s" % ", ".join(sorted(DEPTH_DELIVERY_FORMATS)))
        dopt = GsrDepthDeliveryOptions(DEPTH_DELIVERY_FORMATS[depth], int(depth_step), float(near), 0)
        self._check(self._L.gsr_comm_set_depth(self._ctx, ctypes.byref(dopt)))

    def frame_depth_layout(self):
        """The gathered plane (gsr_frame_depth_layout): depth_layout()'s fields, offset 0."""
        lay = GsrDepthLayout()
        self._check(self._L.gsr_frame_depth_layout(self._ctx, ctypes.byref(lay)))
        names = {v: k for k, v in DEPTH_DELIVERY_FORMATS.items()}
        return {"format": names[lay.format], "step": lay.step, "width": lay.width, "height": lay.height, "stride": lay.stride,
                "offset": int(lay.offset), "bytes": int(lay.bytes), "near": float(lay.near)}

    def read_frame_depth(self):
        """The gathered plane of the last allgather_frame_async(), [Hd, Wd] float32 or uint16; waits like read_frame() and refuses
        a gathered frame with a stale band like it (GSR_ERR_OVERFLOW on every rank: render and gather again)."""
        lay = GsrDepthLayout()
        self._check(self._L.gsr_frame_depth_layout(self._ctx, ctypes.byref(lay)))
        out = np.empty((lay.height, lay.width), dtype=np.float32 if lay.format == GSR_DEPTH_F32 else np.uint16)
        self._check(self._L.gsr_read_frame_depth(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def frame_depth_ptr(self):
        return self._L.gsr_frame_depth_device_ptr(self._ctx)


def pack_selection(picked):
    """bool[n] -> uint32[ceil(n / 32)], splat i = bit i & 31 of word i >> 5 (the selection's layout)."""
    b = np.ascontiguousarray(picked).reshape(-1) != 0
    return np.packbits(np.concatenate([b, np.zeros(-b.size % 32, dtype=bool)]), bitorder="little").view(np.uint32).copy()


def unpack_selection(words, n):
    """uint32[>= ceil(n / 32)] -> bool[n]."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def new_group_id():
    """128 bytes identifying a new RCCL communicator (rank 0 creates it; the host distributes it)."""
    buf = (ctypes.c_uint8 * GSR_COMM_ID_BYTES)()
    L = load_library()
    rc = L.gsr_comm_unique_id(buf)
    if rc:
        raise GsplatError("gsr_comm_unique_id failed (%d): %s" % (rc, L.gsr_last_error(None).decode()))
    return bytes(buf)


def build_id():
    """Hash of the kernel sources the loaded library was built from."""
    return load_library().gsr_build_id().decode()


WebGLRenderer = HIPRenderer  # the name callers of the reference use (src/index.ts:5)
