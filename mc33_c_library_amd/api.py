"""Python view of the C ABI (include/mc33_hip.h, include/marching_cubes_33.h).

Plumbing only: device memory and streams come from PyTorch-ROCm, the work is done by the HIP kernels
inside libMC33_{f32,f64,u8,u16,u32}.so (one library per grid sample type).  There is no CPU fallback: loading fails loudly when the shared object is
missing, and every call into it fails loudly when no GPU is present.
"""
import collections
import ctypes as C
import math
import os

PKG = os.path.dirname(os.path.abspath(__file__))

OK, EINVAL, ENOGPU, ENOMEM, ECAPACITY, ERUNTIME, EOVERFLOW = 0, -1, -2, -3, -4, -5, -6


class GridDesc(C.Structure):
    _fields_ = [("npx", C.c_uint), ("npy", C.c_uint), ("npz_resident", C.c_uint), ("plane0", C.c_uint),
                ("nz_total", C.c_uint), ("r0", C.c_double * 3), ("d", C.c_double * 3),
                ("sample_bytes", C.c_int), ("device", C.c_int)]


class Range(C.Structure):
    _fields_ = [("z_begin", C.c_uint), ("z_end", C.c_uint), ("ghost_below", C.c_uint), ("id_base", C.c_uint)]


class Counts(C.Structure):
    _fields_ = [("nV", C.c_ulonglong), ("nT", C.c_ulonglong), ("nV_ghost", C.c_ulonglong),
                ("nT_ghost", C.c_ulonglong), ("active_cells", C.c_ulonglong)]


class Timing(C.Structure):
    _fields_ = [("sweep_ms", C.c_float), ("scan_ms", C.c_float), ("emit_ms", C.c_float), ("total_ms", C.c_float),
                ("sweep_launches", C.c_uint)]


class Measures(C.Structure):
    _fields_ = [("nV", C.c_ulonglong), ("nT", C.c_ulonglong), ("area", C.c_double), ("volume", C.c_double),
                ("moment", C.c_double * 3), ("origin", C.c_double * 3), ("bbox_min", C.c_double * 3), ("bbox_max", C.c_double * 3),
                ("property_integral", C.c_double), ("has_property", C.c_int)]


class Component(C.Structure):
    _fields_ = [("root", C.c_uint), ("nV", C.c_uint), ("nT", C.c_uint), ("area", C.c_double), ("volume", C.c_double)]


class Topology(C.Structure):
    _fields_ = [(n, C.c_ulonglong) for n in ("nV", "nT", "referenced_vertices", "edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges",
                                             "degenerate_triangles", "boundary_loops", "components", "closed_components", "genus_sum")] + \
               [("euler", C.c_longlong)] + [(n, C.c_int) for n in ("closed", "manifold", "oriented", "genus_defined")]


class ComponentTopology(C.Structure):
    _fields_ = [("root", C.c_uint), ("nV", C.c_uint), ("nT", C.c_uint)] + \
               [(n, C.c_ulonglong) for n in ("edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges", "degenerate_triangles", "boundary_loops")] + \
               [("euler", C.c_longlong), ("genus", C.c_int)]


class Compaction(C.Structure):
    """mc33hip_compaction (include/mc33_hip.h)"""
    _fields_ = [("V", C.c_void_p), ("N", C.c_void_p), ("T", C.c_void_p), ("label", C.c_void_p), ("nV", C.c_ulonglong), ("nT", C.c_ulonglong),
                ("attr", C.c_void_p * 2), ("n_attr", C.c_uint), ("invert", C.c_int), ("roots", C.c_void_p), ("n_roots", C.c_ulonglong),
                ("oV", C.c_void_p), ("oN", C.c_void_p), ("oT", C.c_void_p), ("oAttr", C.c_void_p * 2), ("oMap", C.c_void_p),
                ("capV", C.c_ulonglong), ("capT", C.c_ulonglong),
                ("nV_out", C.c_ulonglong), ("nT_out", C.c_ulonglong), ("components_kept", C.c_ulonglong)]


class ComponentFilter(C.Structure):
    """mc33_component_filter (include/marching_cubes_33.h); a zeroed one keeps every component"""
    _fields_ = [("min_triangles", C.c_uint), ("min_area", C.c_double), ("min_abs_volume", C.c_double), ("largest", C.c_uint), ("closed_only", C.c_int)]


class Smoothing(C.Structure):
    """mc33hip_smoothing (include/mc33_hip.h)"""
    _fields_ = [("V", C.c_void_p), ("T", C.c_void_p), ("nV", C.c_ulonglong), ("nT", C.c_ulonglong),
                ("iterations", C.c_uint), ("lam", C.c_double), ("mu", C.c_double), ("pin_boundary", C.c_int),
                ("oV", C.c_void_p), ("oN", C.c_void_p),
                ("max_degree", C.c_ulonglong), ("isolated_vertices", C.c_ulonglong), ("boundary_vertices", C.c_ulonglong),
                ("invalid_triangles", C.c_ulonglong)]


class SurfaceSmoothing(C.Structure):
    """mc33_smoothing (include/marching_cubes_33.h)"""
    _fields_ = [("iterations", C.c_uint), ("lam", C.c_double), ("mu", C.c_double), ("pin_boundary", C.c_int)]


class Simplification(C.Structure):
    """mc33hip_simplification (include/mc33_hip.h)"""
    _fields_ = [("V", C.c_void_p), ("T", C.c_void_p), ("nV", C.c_ulonglong), ("nT", C.c_ulonglong),
                ("attr", C.c_void_p * 2), ("n_attr", C.c_uint), ("origin", C.c_double * 3), ("cell", C.c_double * 3),
                ("mode", C.c_int), ("drop_duplicates", C.c_int),
                ("oV", C.c_void_p), ("oT", C.c_void_p), ("oN", C.c_void_p), ("oAttr", C.c_void_p * 2), ("oMap", C.c_void_p),
                ("capV", C.c_ulonglong), ("capT", C.c_ulonglong)] + \
               [(n, C.c_ulonglong) for n in ("nV_out", "nT_out", "clusters", "max_cluster", "collapsed_triangles", "duplicate_triangles",
                                             "invalid_triangles", "clamped_vertices")]


class SurfaceSimplification(C.Structure):
    """mc33_simplification (include/marching_cubes_33.h); cell in units of the grid spacing"""
    _fields_ = [("cell", C.c_double * 3), ("mode", C.c_int), ("drop_duplicates", C.c_int)]


SIMPLIFY_MODES = {"mean": 0, "first": 1}


class Clipping(C.Structure):
    """mc33hip_clipping (include/mc33_hip.h)"""
    _fields_ = [("V", C.c_void_p), ("N", C.c_void_p), ("T", C.c_void_p), ("nV", C.c_ulonglong), ("nT", C.c_ulonglong),
                ("attr", C.c_void_p * 2), ("n_attr", C.c_uint), ("attr_mode", C.c_int * 2), ("plane", C.c_double * 4),
                ("oV", C.c_void_p), ("oN", C.c_void_p), ("oT", C.c_void_p), ("oAttr", C.c_void_p * 2), ("oMap", C.c_void_p),
                ("capV", C.c_ulonglong), ("capT", C.c_ulonglong)] + \
               [(n, C.c_ulonglong) for n in ("nV_out", "nT_out", "kept_vertices", "cut_vertices", "on_plane_vertices", "whole_triangles", "cut_triangles",
                                             "dropped_triangles", "invalid_triangles", "nonfinite_vertices")]


class SurfaceClip(C.Structure):
    """mc33_clip (include/marching_cubes_33.h): n <= 6 planes a, b, c, w in the coordinates of the vertices; s >= 0 stays"""
    _fields_ = [("n", C.c_uint), ("plane", (C.c_double * 4) * 6)]


CLIP_MODES = {"copy": 0, "lerp_f32": 1}
CLIP_COUNTS = ("nV_out", "nT_out", "kept_vertices", "cut_vertices", "on_plane_vertices", "whole_triangles", "cut_triangles", "dropped_triangles",
               "invalid_triangles", "nonfinite_vertices")


class Capping(C.Structure):
    """mc33hip_capping (include/mc33_hip.h)"""
    _fields_ = [("V", C.c_void_p), ("N", C.c_void_p), ("T", C.c_void_p), ("nV", C.c_ulonglong), ("nT", C.c_ulonglong),
                ("capV", C.c_ulonglong), ("capT", C.c_ulonglong), ("iso", C.c_double), ("lo", C.c_uint * 3), ("hi", C.c_uint * 3), ("invert", C.c_int),
                ("attr", C.c_void_p * 2), ("n_attr", C.c_uint), ("attr_mode", C.c_int * 2)] + \
               [(n, C.c_ulonglong) for n in ("nV_out", "nT_out", "cap_vertices", "cap_triangles", "rim_segments", "capped_cells", "skipped_cells", "off_face_edges",
                                             "invalid_triangles", "nonfinite_vertices")] + [("solid_above", C.c_int), ("closed", C.c_int)]


class SurfaceCap(C.Structure):
    """mc33_cap (include/marching_cubes_33.h): the box in grid points (hi all 0: the whole grid) and invert"""
    _fields_ = [("lo", C.c_uint * 3), ("hi", C.c_uint * 3), ("invert", C.c_int)]


class SurfaceCapInfo(C.Structure):
    """mc33_cap_info (include/marching_cubes_33.h)"""
    _fields_ = [(n, C.c_uint) for n in ("nV", "nT", "cap_vertices", "cap_triangles", "rim_segments", "capped_cells", "skipped_cells", "off_face_edges")] + \
               [("solid_above", C.c_int), ("closed", C.c_int)]


CAP_MODES = {"word": 0, "f32": 1}
CAP_COUNTS = ("nV_out", "nT_out", "cap_vertices", "cap_triangles", "rim_segments", "capped_cells", "skipped_cells", "off_face_edges", "invalid_triangles",
              "nonfinite_vertices", "solid_above", "closed")


class Rendering(C.Structure):
    """mc33hip_rendering (include/mc33_hip.h)"""
    _fields_ = [("V", C.c_void_p), ("N", C.c_void_p), ("T", C.c_void_p), ("C", C.c_void_p), ("nV", C.c_ulonglong), ("nT", C.c_ulonglong),
                ("m", C.c_double * 16), ("width", C.c_uint), ("height", C.c_uint), ("cull", C.c_int), ("two_sided", C.c_int),
                ("light", C.c_double * 3), ("ambient", C.c_double), ("diffuse", C.c_double), ("base_color", C.c_uint), ("background", C.c_uint),
                ("oRGBA", C.c_void_p), ("oDepth", C.c_void_p), ("oTri", C.c_void_p)] + \
               [(n, C.c_ulonglong) for n in ("drawn", "culled", "degenerate", "rejected", "offscreen", "invalid_triangles", "fragments", "covered")]


class Distance(C.Structure):
    """mc33hip_distance (include/mc33_hip.h)"""
    _fields_ = [("P", C.c_void_p), ("nP", C.c_ulonglong), ("V", C.c_void_p), ("T", C.c_void_p), ("nV", C.c_ulonglong), ("nT", C.c_ulonglong),
                ("signed_distance", C.c_int), ("oDist", C.c_void_p), ("oTri", C.c_void_p), ("oPoint", C.c_void_p)] + \
               [(n, C.c_ulonglong) for n in ("matched_points", "unmatched_points", "invalid_triangles", "nonfinite_triangles")] + \
               [(n, C.c_double) for n in ("max", "min", "sum", "sum_sq")] + [("argmax", C.c_ulonglong), ("argmin", C.c_ulonglong)] + \
               [("lattice", C.c_uint * 3), ("triangle_tests", C.c_ulonglong)]


class SurfaceDistance(C.Structure):
    """mc33_distance (include/marching_cubes_33.h)"""
    _fields_ = [("points", C.c_ulonglong), ("unmatched", C.c_ulonglong), ("max", C.c_double), ("min", C.c_double), ("mean", C.c_double), ("rms", C.c_double),
                ("argmax", C.c_uint)]


DISTANCE_FIELDS = ("matched_points", "unmatched_points", "invalid_triangles", "nonfinite_triangles", "max", "min", "sum", "sum_sq", "argmax", "argmin",
                   "triangle_tests")


class View(C.Structure):
    """mc33_view (include/marching_cubes_33.h): what DeviceGrid.render takes for its view, too"""
    _fields_ = [("m", C.c_double * 16), ("width", C.c_uint), ("height", C.c_uint), ("cull", C.c_int), ("two_sided", C.c_int),
                ("light", C.c_double * 3), ("ambient", C.c_double), ("diffuse", C.c_double), ("background", C.c_uint)]


class Image(C.Structure):
    """mc33_image (include/marching_cubes_33.h)"""
    _fields_ = [("width", C.c_uint), ("height", C.c_uint), ("rgba", C.POINTER(C.c_uint)), ("depth", C.POINTER(C.c_float)), ("triangle", C.POINTER(C.c_uint))] + \
               [(n, C.c_uint) for n in ("drawn", "culled", "degenerate", "rejected", "offscreen", "invalid_triangles")] + \
               [("fragments", C.c_ulonglong), ("covered", C.c_ulonglong), ("nV", C.c_uint), ("nT", C.c_uint)]


RENDER_COUNTS = ("drawn", "culled", "degenerate", "rejected", "offscreen", "invalid_triangles", "fragments", "covered")
IMAGE_RGBA, IMAGE_DEPTH, IMAGE_IDS = 1, 2, 4


class Sectioning(C.Structure):
    """mc33hip_section (include/mc33_hip.h)"""
    _fields_ = [("V", C.c_void_p), ("T", C.c_void_p), ("nV", C.c_ulonglong), ("nT", C.c_ulonglong),
                ("attr", C.c_void_p * 2), ("n_attr", C.c_uint), ("attr_mode", C.c_int * 2), ("plane", C.c_double * 4),
                ("oP", C.c_void_p), ("oS", C.c_void_p), ("oAttr", C.c_void_p * 2), ("oLabel", C.c_void_p), ("oNext", C.c_void_p), ("oPointMap", C.c_void_p),
                ("capP", C.c_ulonglong), ("capS", C.c_ulonglong)] + \
               [(n, C.c_ulonglong) for n in ("nP_out", "nS_out", "on_points", "cut_points", "isolated_points", "degenerate_segments", "crossing_triangles",
                                             "invalid_triangles", "nonfinite_vertices", "contours", "closed_contours", "open_ends", "branch_points")] + \
               [("length", C.c_double), ("area_vector", C.c_double * 3), ("area", C.c_double), ("origin", C.c_double * 3)]


class Contour(C.Structure):
    """mc33hip_contour (include/mc33_hip.h), mc33_contour (include/marching_cubes_33.h): a row of the contour table"""
    _fields_ = [("root", C.c_uint), ("points", C.c_uint), ("segments", C.c_uint), ("open_ends", C.c_uint), ("branch_points", C.c_uint), ("closed", C.c_int),
                ("length", C.c_double), ("area", C.c_double)]


class SurfaceSection(C.Structure):
    """mc33_section (include/marching_cubes_33.h): the malloc blocks of MC33_section_isosurface; MC33_real is float here - the
    double library's P is read through its own pointer type"""
    _fields_ = [("nP", C.c_uint), ("nS", C.c_uint), ("P", C.c_void_p), ("S", C.POINTER(C.c_uint * 2)), ("contour", C.POINTER(C.c_uint)), ("next", C.POINTER(C.c_uint)),
                ("color", C.POINTER(C.c_int))] + \
               [(n, C.c_uint) for n in ("on_points", "cut_points", "contours", "closed_contours", "open_ends", "branch_points", "degenerate_segments")] + \
               [("length", C.c_double), ("area", C.c_double), ("plane", C.c_double * 4)]


class SectionLevel(C.Structure):
    """mc33_section_level (include/marching_cubes_33.h): one plane of MC33_section_profile"""
    _fields_ = [("segments", C.c_ulonglong), ("length", C.c_double), ("area", C.c_double)]


SECTION_COUNTS = ("nP_out", "nS_out", "on_points", "cut_points", "isolated_points", "degenerate_segments", "crossing_triangles", "invalid_triangles",
                  "nonfinite_vertices", "contours", "closed_contours", "open_ends", "branch_points")


class Resampling(C.Structure):
    """mc33hip_resampling (include/mc33_hip.h): taps are HOST arrays of doubles, NULL = the single tap 1.0"""
    _fields_ = [("taps", C.POINTER(C.c_double) * 3), ("ntaps", C.c_uint * 3), ("stride", C.c_uint * 3)]


class GridResampling(C.Structure):
    """mc33_resampling (include/marching_cubes_33.h); sigma in samples, radius 0 = ceil(3 sigma)"""
    _fields_ = [("sigma", C.c_double * 3), ("radius", C.c_uint * 3), ("stride", C.c_uint * 3)]


class Ranking(C.Structure):
    """mc33hip_ranking (include/mc33_hip.h) and mc33_ranking (include/marching_cubes_33.h): radius per axis x, y, z; rank RANK_*"""
    _fields_ = [("radius", C.c_uint * 3), ("rank", C.c_int)]


RANK_MIN, RANK_MEDIAN, RANK_MAX = 0, 1, 2
RANKS = {"min": RANK_MIN, "median": RANK_MEDIAN, "max": RANK_MAX}


class Spectrum(C.Structure):
    """mc33hip_spectrum (include/mc33_hip.h): isos, cut_cells and histogram are HOST arrays"""
    _fields_ = [("isos", C.POINTER(C.c_double)), ("n", C.c_uint), ("cut_cells", C.POINTER(C.c_ulonglong)), ("histogram", C.POINTER(C.c_ulonglong)),
                ("points", C.c_ulonglong), ("cells", C.c_ulonglong), ("nan_samples", C.c_ulonglong),
                ("sample_min", C.c_double), ("sample_max", C.c_double)]


class SpectrumInfo(C.Structure):
    """mc33_spectrum_info (include/marching_cubes_33.h)"""
    _fields_ = [("points", C.c_ulonglong), ("cells", C.c_ulonglong), ("nan_samples", C.c_ulonglong),
                ("sample_min", C.c_double), ("sample_max", C.c_double)]


class Curvature(C.Structure):
    """mc33hip_curvature (include/mc33_hip.h): dV and the four outputs are DEVICE arrays, each output may be NULL"""
    _fields_ = [("dV", C.c_void_p), ("nV", C.c_ulonglong), ("sign", C.c_int),
                ("oMean", C.c_void_p), ("oGauss", C.c_void_p), ("oK1", C.c_void_p), ("oK2", C.c_void_p),
                ("lo", C.c_double * 4), ("hi", C.c_double * 4), ("finite", C.c_ulonglong), ("undefined", C.c_ulonglong)]


class IsosurfaceCurvature(C.Structure):
    """mc33_curvature (include/marching_cubes_33.h)"""
    _fields_ = [("nV", C.c_uint), ("nT", C.c_uint), ("lo", C.c_double * 4), ("hi", C.c_double * 4),
                ("finite", C.c_ulonglong), ("undefined", C.c_ulonglong), ("total_mean", C.c_double), ("total_gauss", C.c_double)]


CURVATURES = ("mean", "gauss", "k1", "k2")

# Every ctypes.Structure above and the C type it mirrors (a class that mirrors two identical structs has two rows);
# tests/test_bindings_cpu.py compares size and every field with the compiler.  FIELD_ALIASES: (class, field) -> C member where
# the names differ ("lambda" cannot be read as a Python attribute).
STRUCTS = {
    "mc33hip_grid_desc": GridDesc, "mc33hip_range": Range, "mc33hip_counts": Counts, "mc33hip_timing": Timing,
    "mc33hip_measures": Measures, "mc33hip_component": Component, "mc33_component": Component,
    "mc33hip_topology": Topology, "struct mc33hip_component_topology": ComponentTopology, "mc33_component_topology": ComponentTopology,
    "mc33hip_compaction": Compaction, "mc33_component_filter": ComponentFilter,
    "mc33hip_smoothing": Smoothing, "mc33_smoothing": SurfaceSmoothing,
    "mc33hip_simplification": Simplification, "mc33_simplification": SurfaceSimplification,
    "mc33hip_clipping": Clipping, "mc33_clip": SurfaceClip,
    "mc33hip_capping": Capping, "mc33_cap": SurfaceCap, "mc33_cap_info": SurfaceCapInfo,
    "mc33hip_rendering": Rendering, "mc33_view": View, "mc33_image": Image,
    "mc33hip_distance": Distance, "mc33_distance": SurfaceDistance,
    "mc33hip_section": Sectioning, "mc33hip_contour": Contour, "mc33_contour": Contour, "mc33_section": SurfaceSection,
    "mc33_section_level": SectionLevel,
    "mc33hip_resampling": Resampling, "mc33_resampling": GridResampling,
    "mc33hip_ranking": Ranking, "mc33_ranking": Ranking,
    "mc33hip_spectrum": Spectrum, "mc33_spectrum_info": SpectrumInfo,
    "mc33hip_curvature": Curvature, "mc33_curvature": IsosurfaceCurvature,
}
FIELD_ALIASES = {(Smoothing, "lam"): "lambda", (SurfaceSmoothing, "lam"): "lambda"}

# name -> (restype, argtypes, optional): what load_library declares of the device-level ABI (include/mc33_hip.h) and of the host C
# helpers of include/marching_cubes_33.h that this module calls.  optional: MC33_LIB_DIR may name an older build without it.
# tests/test_bindings_cpu.py compares every row with the headers.
_P, _V, _I, _U, _D, _Q, _Z = C.POINTER, C.c_void_p, C.c_int, C.c_uint, C.c_double, C.c_ulonglong, C.c_size_t
SIGNATURES = {
    "mc33hip_set_id_base": (_I, [_V, _U], False),
    "mc33hip_create": (_I, [_P(_V), _P(GridDesc)], False),
    "mc33hip_destroy": (None, [_V], False),
    "mc33hip_last_error": (C.c_char_p, [], False),
    "mc33hip_upload_rows": (_I, [_V, _V], False),
    "mc33hip_upload_contiguous": (_I, [_V, _V], False),
    "mc33hip_adopt_device": (_I, [_V, _V, _Z, _Z], False),
    "mc33hip_set_stream": (_I, [_V, _V], False),
    "mc33hip_count": (_I, [_V, _D, _P(Range), _P(Counts)], False),
    "mc33hip_emit": (_I, [_V, _V, _V, _V, _Q, _Q], False),
    "mc33hip_extract": (_I, [_V, _D, _P(Range), _V, _V, _V, _Q, _Q, _P(Counts)], False),
    "mc33hip_last_timing": (_I, [_V, _P(Timing)], False),
    "mc33hip_download": (_I, [_V, _V, _V, _Z], False),
    "mc33hip_device_alloc": (_I, [_V, _P(_V), _Z], False),
    "mc33hip_device_free": (_I, [_V, _V], False),
    "mc33hip_set_inclined": (_I, [_V, _V, _V, _I], False),
    "mc33hip_download_concurrent": (_I, [_V, _V, _V, _Z], False),
    "mc33hip_synchronize": (_I, [_V], False),
    "mc33hip_download_many": (_I, [_V, _I, _P(_V), _P(_V), _P(_Z), _I], False),
    "mc33hip_set_normal_neg": (_I, [_V, _I], False),
    "mc33hip_sweep_many": (_I, [_V, _P(_D), _I, _P(Range)], False),
    "mc33hip_set_timing": (_I, [_V, _I], False),
    "mc33hip_probe_read": (_I, [_V, _I, _P(C.c_float), _P(C.c_float), _P(_Q)], False),
    "mc33hip_prepare_many": (_I, [_V, _P(_D), _I, _P(Range)], False),
    "mc33hip_emit_download": (_I, [_V, _V, _V, _V, _Q, _Q, _V, _V, _V], False),
    "mc33hip_download_wait": (_I, [_V], False),
    "mc33hip_own_stream": (_I, [_V], False),
    "mc33hip_device_count": (_I, [], False),
    "mc33hip_count_async": (_I, [_V, _D, _P(Range)], False),
    "mc33hip_counts_to_device": (_I, [_V, _V], False),
    "mc33hip_bases_from_table": (_I, [_V, _V, _I, _I, _I], False),
    "mc33hip_emit_at_device_bases": (_I, [_V, _V, _V, _V, _Q, _Q], False),
    "mc33hip_count_finish": (_I, [_V, _P(Counts)], False),
    "mc33hip_property_upload_rows": (_I, [_V, _V, _U, _U], False),
    "mc33hip_property_upload_contiguous": (_I, [_V, _V, _U, _U], False),
    "mc33hip_property_adopt_device": (_I, [_V, _V, _Z, _Z, _U, _U], False),
    "mc33hip_property_drop": (_I, [_V], False),
    "mc33hip_sample_property": (_I, [_V, _V, _Q, _V], False),
    "mc33hip_color_vertices": (_I, [_V, _V, _Q, _P(_I), _U, _D, _D, _I, _V], False),
    "mc33hip_download_enqueue": (_I, [_V, _V, _V, _Z], False),
    "mc33hip_measure_surface": (_I, [_V, _V, _Q, _V, _Q, _V, _P(Measures)], False),
    "mc33hip_label_components": (_I, [_V, _V, _Q, _Q, _V, _P(_Q), _P(_Q)], False),
    "mc33hip_measure_components": (_I, [_V, _V, _Q, _V, _Q, _V, _V, _Q, _P(_Q)], False),
    "mc33hip_surface_topology": (_I, [_V, _V, _Q, _Q, _P(Topology)], False),
    "mc33hip_component_topology": (_I, [_V, _V, _Q, _Q, _V, _V, _Q, _P(_Q)], False),
    "mc33hip_compact_components": (_I, [_V, _P(Compaction)], False),
    "mc33hip_smooth_surface": (_I, [_V, _P(Smoothing)], False),
    "mc33hip_vertex_normals": (_I, [_V, _V, _Q, _V, _Q, _V], False),
    "mc33hip_smooth_timing": (_I, [_V, _P(C.c_float), _P(C.c_float), _P(C.c_float), _U, _P(_U)], False),
    "mc33hip_simplify_surface": (_I, [_V, _P(Simplification)], False),
    "mc33hip_resampled_size": (_I, [_V, _P(Resampling), _P(_U * 3)], False),
    "mc33hip_resample_grid": (_I, [_V, _P(Resampling), _V, _Z, _Z], False),
    "mc33hip_context_device": (_I, [_V], False),
    "mc33hip_rank_grid": (_I, [_V, _P(Ranking), _V, _Z, _Z], False),
    "mc33hip_grid_spectrum": (_I, [_V, _P(Range), _P(Spectrum)], False),
    "mc33hip_clip_surface": (_I, [_V, _P(Clipping)], False),
    "mc33hip_section_surface": (_I, [_V, _P(Sectioning)], False),
    "mc33hip_section_contours": (_I, [_V, _V, _Q, _V, _Q, _V, _P(_D * 4), _V, _Q, _P(_Q)], False),
    "mc33hip_section_ladder": (_I, [_V, _V, _Q, _V, _Q, _P(_D * 3), _P(_D), _U, _P(_Q), _P(_D), _P(_D), _P(_Q)], False),
    "mc33hip_grid_stable": (_I, [_V, _I], True),  # (every grid is volatile in a build without it)
    "mc33hip_grid_changed": (_I, [_V], True),
    "mc33hip_range_table": (_I, [_V, _V, _Z], True),
    "mc33hip_sweep_skipped": (_I, [_V, _P(_Q * 3)], True),
    "mc33hip_sweep_plan": (_I, [_V, _V, _Z, _P(_Q * 3)], True),
    "mc33hip_sweep_plan_weight": (_I, [_V, _P(_D)], True),
    "mc33hip_sweep_live": (_I, [_V, _V, _Z, _P(_Q * 2)], True),
    "mc33hip_sweep_packed": (_I, [_V, _V, _Z, _P(_Q * 3)], True),
    "mc33hip_range_blocks": (_I, [_V, _V, _Z], True),
    "mc33hip_block_words": (_I, [_V, _V, _Z], True),
    "mc33hip_alias_cells": (_I, [_V, _P(_Q)], True),
    "mc33hip_sweep_skipped_blocks": (_I, [_V, _P(_Q * 3)], True),
    "mc33hip_emit_shape": (_I, [_V, _P(_Q * 8)], True),
    "mc33hip_tail_shape": (_I, [_V, _P(_Q * 8)], True),
    "mc33hip_list_counts": (_I, [_V, _P(_U), _P(_U), _Z], True),
    "mc33hip_curvature_vertices": (_I, [_V, _P(Curvature)], True),
    "mc33hip_color_values": (_I, [_V, _V, _Q, _P(_I), _U, _D, _D, _I, _V], True),
    "mc33hip_cap_surface": (_I, [_V, _P(Capping)], True),
    "mc33hip_render_surface": (_I, [_V, _P(Rendering)], True),
    "mc33hip_render_timing": (_I, [_V, _P(C.c_float * 6)], True),
    "mc33hip_surface_distance": (_I, [_V, _P(Distance)], True),
    "mc33hip_distance_timing": (_I, [_V, _P(C.c_float * 3)], True),
    "MC33_select_components": (_I, [_V, _V, _U, _P(ComponentFilter), _V], False),
    "MC33_gaussian_taps": (_I, [_D, _U, _P(_D)], False),
    "MC33_isovalue_ladder": (_I, [_D, _D, _U, _V], False),
    "MC33_clip_box": (_I, [_P(_D * 3), _P(_D * 3), _P(SurfaceClip)], False),
}
HIP_API = [name for name in SIGNATURES if name.startswith("mc33hip_")]
REFERENCE_API = ["create_MC33", "calculate_isosurface", "size_of_isosurface", "free_MC33", "free_surface_memory",
                 "adjustvectorlenght_s", "DefaultColorMC", "free_memory_grd", "alloc_F", "grid_from_data_pointer",
                 "generate_grid_from_fn", "_multTSA_bf", "_multA_bf", "mult_Abf",
                 "write_bin_s", "read_bin_s", "write_txt_s", "write_obj_s", "write_ply_s",
                 "read_grd", "read_grd_binary", "read_scanfiles", "read_raw_file", "read_dat_file", "calculate_isosurfaces", "MC33_grid_changed",
                 "MC33_set_property_grid", "MC33_set_color_map",
                 "MC33_measure_isosurface", "MC33_measure_isosurfaces", "MC33_measure_components",
                 "MC33_isosurface_topology", "MC33_component_topology",
                 "MC33_select_components", "MC33_calculate_filtered_isosurface", "MC33_calculate_smoothed_isosurface",
                 "MC33_calculate_simplified_isosurface",
                 "MC33_gaussian_taps", "MC33_create_resampled", "MC33_resampled_grid", "MC33_create_ranked",
                 "MC33_grid_spectrum", "MC33_isovalue_ladder",
                 "MC33_calculate_clipped_isosurface", "MC33_clip_box",
                 "MC33_section_isosurface", "MC33_free_section", "MC33_section_contours", "MC33_section_profile",
                 "MC33_set_color_source", "MC33_isosurface_curvature",
                 "MC33_calculate_capped_isosurface",
                 "MC33_render_isosurface", "MC33_free_image", "MC33_view_fit", "MC33_write_image_ppm",
                 "MC33_isosurface_distance", "MC33_simplification_error"]


# what DeviceGrid.emit_shape() returns: out[8] of mc33hip_emit_shape (slow_kernel: 0 a thread per record, 1 a lane per slot, 2 left out)
EmitShape = collections.namedtuple("EmitShape", "records slow_records batches vertex_blocks triangle_blocks slow_blocks slow_kernel triangles_first")
# what DeviceGrid.tail_shape() returns: out[8] of mc33hip_tail_shape
TailShape = collections.namedtuple("TailShape", "nslots groups shift scan_chunks grouped slots_blocks slow_total dirty_total")


class MC33Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mc33hip error %d: %s" % (code, msg))
        self.code = code


def library_path(dtype="f32"):
    # MC33_LIB_DIR: developer switch (tools/): load a -DMC33_DEV build from another directory
    return os.path.join(os.environ.get("MC33_LIB_DIR") or PKG, "libMC33_%s.so" % dtype)


_libs = {}


def load_library(dtype="f32"):
    """dlopen the product library; raises if it was not built (python -m mc33_c_library_amd.build)."""
    if dtype in _libs:
        return _libs[dtype]
    path = library_path(dtype)
    if not os.path.exists(path):
        raise FileNotFoundError("%s not built - run `python -m mc33_c_library_amd.build` (hipcc, gfx950); "
                                "there is no CPU fallback" % path)
    try:  # torch's bundled HIP runtime must be the one the process loads first (same SONAME)
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(path)
    for name, (restype, argtypes, optional) in SIGNATURES.items():
        if optional and not hasattr(lib, name):  # (MC33_LIB_DIR may name an older build, for a comparison side by side)
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _libs[dtype] = lib
    return lib


def gaussian_taps(sigma, radius=0):
    """The 2 r + 1 weights of a Gaussian of `sigma` samples cut off at `radius` (0: ceil(3 sigma), at least 1; sigma 0: the single
    tap 1.0) as a list of floats - the library's MC33_gaussian_taps (include/marching_cubes_33.h), host C that needs no GPU: there
    is no second implementation.  ValueError for what it refuses: a negative, NaN or infinite sigma, a radius above 8."""
    lib = load_library("f32")
    taps = (C.c_double * 17)()
    try:
        r = lib.MC33_gaussian_taps(float(sigma), int(radius), taps)
    except (C.ArgumentError, OverflowError):
        r = -1
    if r < 0:
        raise ValueError("MC33_gaussian_taps refused sigma=%r radius=%r" % (sigma, radius))
    return [taps[k] for k in range(2 * r + 1)]


def isovalue_ladder(lo, hi, n, dtype="f32"):
    """n isovalues strictly between lo and hi, (MC33_real)(lo + (hi - lo) * (k + 1) / (n + 1)), as a list of floats - the
    library's MC33_isovalue_ladder (include/marching_cubes_33.h), host C that needs no GPU: there is no second implementation.
    dtype: the grid's sample type (MC33_real is double for "f64", float otherwise).  ValueError for what it refuses: bounds that
    are not finite, lo >= hi, n > 255, steps that MC33_real does not tell apart."""
    lib = load_library(dtype)
    out = ((C.c_double if dtype == "f64" else C.c_float) * 256)()
    try:
        r = lib.MC33_isovalue_ladder(float(lo), float(hi), int(n), C.cast(out, C.c_void_p))
    except (C.ArgumentError, OverflowError, TypeError, ValueError):
        r = -1
    if r < 0:
        raise ValueError("MC33_isovalue_ladder refused lo=%r hi=%r n=%r" % (lo, hi, n))
    return [float(out[k]) for k in range(r)]


def clip_box(lo, hi):
    """The six planes (a, b, c, w) that keep the box [lo, hi], in the order x - lo[0], hi[0] - x, y - lo[1], hi[1] - y, z - lo[2],
    hi[2] - z, as a list of 4-tuples of floats - the library's MC33_clip_box (include/marching_cubes_33.h), host C that needs no
    GPU: there is no second implementation.  ValueError for what it refuses: a bound that is not finite, lo >= hi on an axis."""
    lib = load_library("f32")
    out = SurfaceClip()
    try:
        r = lib.MC33_clip_box(C.byref((C.c_double * 3)(*[float(x) for x in lo])), C.byref((C.c_double * 3)(*[float(x) for x in hi])), C.byref(out))
    except (C.ArgumentError, OverflowError, TypeError, ValueError):
        r = -1
    if r != 0:
        raise ValueError("MC33_clip_box refused lo=%r hi=%r" % (lo, hi))
    return [tuple(out.plane[k][j] for j in range(4)) for k in range(out.n)]


class SectionResult:
    """What DeviceGrid.section returns (include/mc33_hip.h: mc33hip_section_surface): P, S, attrs, label, next, point_map (device
    tensors), plane, info (the dict of the thirteen counts), length, area_vector, area, origin."""

    def __init__(self, a, P, S, attrs, label, nxt, pmap):
        self.P, self.S, self.attrs, self.label, self.next, self.point_map = P, S, attrs, label, nxt, pmap
        self.plane = tuple(a.plane)
        self.info = {n: int(getattr(a, n)) for n in SECTION_COUNTS}
        self.length, self.area, self.area_vector, self.origin = a.length, a.area, tuple(a.area_vector), tuple(a.origin)


class GridSpectrum:
    """What DeviceGrid.spectrum returns (include/mc33_hip.h: mc33hip_grid_spectrum): isovalues (the doubles that were passed),
    cut_cells (numpy uint64 [n]: cells the surface of isovalue k cuts), histogram (numpy uint64 [n + 1]: grid points above exactly
    j of the isovalues), points, cells, nan_samples, sample_min, sample_max."""

    def __init__(self, isovalues, cut_cells, histogram, points, cells, nan_samples, sample_min, sample_max):
        self.isovalues, self.cut_cells, self.histogram = list(isovalues), cut_cells, histogram
        self.points, self.cells, self.nan_samples = int(points), int(cells), int(nan_samples)
        self.sample_min, self.sample_max = float(sample_min), float(sample_max)

    def busiest(self):
        """the isovalue whose surface cuts the most cells (None without isovalues)"""
        return self.isovalues[int(self.cut_cells.argmax())] if len(self.isovalues) else None

    def __repr__(self):
        return "GridSpectrum(n=%d, points=%d, cells=%d, nan_samples=%d, range=[%r, %r])" % (
            len(self.isovalues), self.points, self.cells, self.nan_samples, self.sample_min, self.sample_max)


class VertexCurvature:
    """What DeviceGrid.curvature returns: the chosen float32 device tensors mean, gauss, k1, k2 [n] (None where not asked for) and
    the summary - lo / hi: {name: extreme of the finite values of that output} (+inf / -inf when it has none, whether or not its
    tensor was asked for); finite: the vertices whose four values are all finite; undefined: the others."""

    def __init__(self, a, tensors):
        self.mean, self.gauss, self.k1, self.k2 = (tensors.get(k) for k in CURVATURES)
        self.lo = {k: a.lo[q] for q, k in enumerate(CURVATURES)}
        self.hi = {k: a.hi[q] for q, k in enumerate(CURVATURES)}
        self.finite, self.undefined = int(a.finite), int(a.undefined)

    def __repr__(self):
        return "VertexCurvature(finite=%d, undefined=%d, mean in [%g, %g], gauss in [%g, %g])" % (
            self.finite, self.undefined, self.lo["mean"], self.hi["mean"], self.lo["gauss"], self.hi["gauss"])


class SurfaceMeasures:
    """What DeviceGrid.measure returns: nV, nT, area, volume (signed, with the winding of T), moment and origin (the area
    centroid is origin + moment / area: `centroid`), bbox_min, bbox_max, property_integral, has_property."""

    def __init__(self, m):
        self.nV, self.nT, self.area, self.volume = int(m.nV), int(m.nT), m.area, m.volume
        self.moment, self.origin = tuple(m.moment), tuple(m.origin)
        self.bbox_min, self.bbox_max = tuple(m.bbox_min), tuple(m.bbox_max)
        self.property_integral, self.has_property = m.property_integral, int(m.has_property)

    @property
    def centroid(self):
        return tuple(o + (q / self.area if self.area else float("nan")) for o, q in zip(self.origin, self.moment))

    def __repr__(self):
        return "SurfaceMeasures(nV=%d, nT=%d, area=%r, volume=%r, centroid=%r)" % (self.nV, self.nT, self.area, self.volume, self.centroid)


class SurfaceTopology:
    """What DeviceGrid.topology returns - the fields of mc33hip_topology (include/mc33_hip.h) as Python ints: nV, nT,
    referenced_vertices, edges, boundary_edges, nonmanifold_edges, misoriented_edges, degenerate_triangles, boundary_loops,
    components, closed_components, genus_sum, euler, and the flags closed, manifold (edge-manifold), oriented, genus_defined."""
    FIELDS = tuple(n for n, _ in Topology._fields_)

    def __init__(self, t):
        for n in self.FIELDS:
            setattr(self, n, int(getattr(t, n)))

    def as_tuple(self):
        return tuple(getattr(self, n) for n in self.FIELDS)

    def __eq__(self, other):
        return isinstance(other, SurfaceTopology) and self.as_tuple() == other.as_tuple()

    def __repr__(self):
        return "SurfaceTopology(%s)" % ", ".join("%s=%d" % (n, getattr(self, n)) for n in self.FIELDS)


def _assert_readable(tensor, npx, whole_words):
    """The readable extent mc33hip_adopt_device asks for (include/mc33_hip.h), checked on the last row of the last plane against
    the tensor's storage (every other row is followed by memory of the same storage): its npx samples and, whole_words, what
    follows them up to the next 4-byte (16-byte) boundary where base, pitch and slice are all multiples of 4 (16) bytes - never
    beyond the pitch."""
    sb = tensor.element_size()
    row = tensor.data_ptr() + ((tensor.shape[0] - 1) * tensor.stride(0) + (tensor.shape[1] - 1) * tensor.stride(1)) * sb
    end = row + npx * sb
    if whole_words:
        terms = (tensor.data_ptr(), tensor.stride(1) * sb, tensor.stride(0) * sb)
        word = 16 if all(t % 16 == 0 for t in terms) else 4 if all(t % 4 == 0 for t in terms) else 1
        end = min(row + tensor.stride(1) * sb, -(-end // word) * word)
    st = tensor.untyped_storage()
    assert end <= st.data_ptr() + st.nbytes(), \
        "the last row of the buffer is read in whole 4- / 16-byte words (include/mc33_hip.h: readable extent): %d bytes behind " \
        "its last sample are not part of the tensor's storage" % (end - st.data_ptr() - st.nbytes())


def _check(lib, rc, allow=()):
    if rc != OK and rc not in allow:
        raise MC33Error(rc, lib.mc33hip_last_error().decode(errors="replace"))
    return rc


class DeviceGrid:
    """A grid (or a z-slab of one) resident in HBM as a torch tensor [planes, rows, pitch], plus the
    extraction context working on it.  dtype float32 or uint16 (carried as torch.int16 bit patterns).
    The tensor is used in place with its strides: any stride(1) >= npx, any stride(0) >= stride(1) * rows, any storage offset
    (include/mc33_hip.h, mc33hip_adopt_device: which alignment allows which kernel form, and what must be readable behind the
    last row); npx: the grid's points per row when the tensor's rows are wider.

    Who must say what when samples change.  The library may keep a table of sample ranges over the grid and leave out the parts of
    the volume that cannot hold the isovalue (include/mc33_hip.h: mc33hip_grid_stable) - only over samples it knows to be
    unchanged.  This class declares the tensor stable and keeps that true with torch's own bookkeeping: before every call that
    classifies samples (count, count_async, sweep_many, prepare_many, extract_into, and everything built on them) it compares
    tensor._version with the value it saw last and tells the library when it differs.  So:
      - a write torch counts - t[...] = x, t.neg_(), t.copy_(...), an out= argument, through any view or detach() of the tensor,
        which share the counter - is seen by the next call with nothing said;
      - a write torch does NOT count needs grid.changed() before the next call: t.data[...] = x, a foreign kernel or library given
        data_ptr(), another DeviceGrid's resample_into(out) when out is this grid's tensor;
      - volatile=True never declares the tensor stable: every call reads the whole grid, as an adopted buffer always did.  A
        tensor whose _version cannot be read (inference tensors) is volatile by itself.
    The table is made by the second sweep since the samples last changed - one extra pass over the grid, once; a grid extracted
    once, or rewritten before every extraction, never pays for it."""

    def __init__(self, tensor, nz_total=None, plane0=0, r0=(0.0, 0.0, 0.0), d=(1.0, 1.0, 1.0), npx=None, volatile=False):
        import torch
        assert tensor.is_cuda and tensor.dim() == 3 and tensor.stride(2) == 1, "need a device tensor [z, y, x]"
        if tensor.dtype == torch.float32:
            self.dtype, sb = "f32", 4
        elif tensor.dtype in (torch.int16, torch.uint16):
            self.dtype, sb = "u16", 2
        elif tensor.dtype == torch.uint8:
            self.dtype, sb = "u8", 1
        elif tensor.dtype in (torch.int32, torch.uint32):
            self.dtype, sb = "u32", 4
        elif tensor.dtype == torch.float64:
            self.dtype, sb = "f64", 8
        else:
            raise TypeError("grid samples must be float32, float64, uint8, (u)int16 or (u)int32 bit patterns")
        self.lib = load_library(self.dtype)
        self.tensor = tensor  # keeps the memory alive
        npz, npy, pitch = tensor.shape[0], tensor.shape[1], tensor.stride(1)
        npx = npx if npx is not None else tensor.shape[2]
        assert 2 <= npx <= tensor.shape[2], "npx: the grid's points per row, at most the tensor's width"
        _assert_readable(tensor, npx, True)
        desc = GridDesc(npx, npy, npz, plane0, (nz_total if nz_total is not None else npz - 1),
                        (C.c_double * 3)(*r0), (C.c_double * 3)(*d), sb, tensor.device.index)
        self.desc = desc
        self.ctx = C.c_void_p()
        _check(self.lib, self.lib.mc33hip_create(C.byref(self.ctx), C.byref(desc)))
        # (per-pass hipEvent timing is off, as in the library: a caller that wants timing() says set_timing(2) first -
        # the event records cost ~20 us per call; MC33_HIP_TIMING in the environment sets the level a context starts with)
        _check(self.lib, self.lib.mc33hip_adopt_device(self.ctx, C.c_void_p(tensor.data_ptr()), pitch, tensor.stride(0)))
        self.device = tensor.device
        self.use_stream(torch.cuda.current_stream(self.device))
        self._version = None  # tensor._version when the samples were last known to be what the library has seen; None: volatile
        if not volatile and hasattr(self.lib, "mc33hip_grid_stable"):
            try:
                self._version = tensor._version
                _check(self.lib, self.lib.mc33hip_grid_stable(self.ctx, 1))
            except RuntimeError:  # (inference tensors do not track versions)
                self._version = None

    def changed(self):
        """The samples were written by a road torch does not count (see the class docstring): forget what was derived from them."""
        if hasattr(self.lib, "mc33hip_grid_changed"):
            _check(self.lib, self.lib.mc33hip_grid_changed(self.ctx))
        if self._version is not None:
            self._version = self.tensor._version

    def _fresh(self):
        """Before every call that sweeps: a write torch has counted since the last look means the samples changed."""
        if self._version is not None and self.tensor._version != self._version:
            self.changed()

    def set_timing(self, level):
        """0: no events (the production path), 1: whole call, 2: per pass (timing() then reports sweep / scan / emit)."""
        _check(self.lib, self.lib.mc33hip_set_timing(self.ctx, int(level)))

    def use_stream(self, stream):
        self.stream = stream
        _check(self.lib, self.lib.mc33hip_set_stream(self.ctx, C.c_void_p(stream.cuda_stream)))

    def set_inclined(self, A=None, Ai=None, triangular=False):
        """Non-orthogonal grid: _GRD._A / _GRD.A_ (3x3, row major); None switches back."""
        if A is None:
            _check(self.lib, self.lib.mc33hip_set_inclined(self.ctx, None, None, 0))
            self.inclined = None
            return
        a = (C.c_double * 9)(*[float(x) for row in A for x in row])
        ai = (C.c_double * 9)(*[float(x) for row in Ai for x in row])
        _check(self.lib, self.lib.mc33hip_set_inclined(self.ctx, a, ai, int(bool(triangular))))
        self.inclined = ([list(row) for row in A], [list(row) for row in Ai], bool(triangular))  # (resampled() hands them on)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.mc33hip_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    def full_range(self):
        return Range(0, self.desc.nz_total, 0, 0)

    def count(self, iso, rng=None):
        self._fresh()
        rng = rng or self.full_range()
        cnt = Counts()
        _check(self.lib, self.lib.mc33hip_count(self.ctx, C.c_double(iso), C.byref(rng), C.byref(cnt)))
        return cnt

    def sweep_many(self, isos, rng=None):
        """Classify up to 8 isovalues in one go (the grid is streamed once per 4 of them); the count / extract calls
        for these isovalues over the same range then skip their sweep."""
        self._fresh()
        rng = rng or self.full_range()
        arr = (C.c_double * len(isos))(*[float(x) for x in isos])
        _check(self.lib, self.lib.mc33hip_sweep_many(self.ctx, arr, len(isos), C.byref(rng)))

    def prepare_many(self, isos, rng=None):
        """sweep_many plus everything else a count needs, every isovalue into buffers of its own: count / emit_into for these
        isovalues then run in any order, any number of times (slabs: all counts first, ONE exchange, then the emits)."""
        self._fresh()
        rng = rng or self.full_range()
        arr = (C.c_double * len(isos))(*[float(x) for x in isos])
        _check(self.lib, self.lib.mc33hip_prepare_many(self.ctx, arr, len(isos), C.byref(rng)))

    def extract_into(self, iso, V, N, T, rng=None):
        """One extraction into caller-owned device tensors V, N [capV,3] float32 and T [capT,3] int32.
        Returns (Counts, enough_capacity)."""
        self._fresh()
        rng = rng or self.full_range()
        cnt = Counts()
        rc = self.lib.mc33hip_extract(self.ctx, C.c_double(iso), C.byref(rng), C.c_void_p(V.data_ptr()),
                                      C.c_void_p(N.data_ptr()), C.c_void_p(T.data_ptr()), V.shape[0], T.shape[0],
                                      C.byref(cnt))
        _check(self.lib, rc, allow=(ECAPACITY,))
        return cnt, rc == OK

    def emit_into(self, V, N, T, id_base=None):
        """Emit pass for the range last counted (asynchronous on the stream)."""
        if id_base is not None:
            _check(self.lib, self.lib.mc33hip_set_id_base(self.ctx, id_base))
        _check(self.lib, self.lib.mc33hip_emit(self.ctx, C.c_void_p(V.data_ptr()), C.c_void_p(N.data_ptr()),
                                               C.c_void_p(T.data_ptr()), V.shape[0], T.shape[0]))

    # -- a z-slab's count, count exchange and emit without a host round trip in between (slabs.py: extract_slab) --------------
    def count_async(self, iso, rng=None):
        """What count() does, enqueued only: the counters stay on the device until count_finish()."""
        self._fresh()
        rng = rng or self.full_range()
        _check(self.lib, self.lib.mc33hip_count_async(self.ctx, C.c_double(iso), C.byref(rng)))

    def counts_to_device(self, dst):
        """{vertices, triangles} of the range last counted into dst, an int64 device tensor of 2 elements (stream-ordered)."""
        import torch
        assert dst.is_cuda and dst.dtype == torch.int64 and dst.numel() >= 2 and dst.is_contiguous()
        _check(self.lib, self.lib.mc33hip_counts_to_device(self.ctx, C.c_void_p(dst.data_ptr())))

    def bases_from_table(self, table, stride, rank, concatenated):
        """table: int64 device tensor, rank r's {vertices, triangles} at table[r * stride]: this rank's vertex id base and output rows."""
        import torch
        assert table.is_cuda and table.dtype == torch.int64 and table.is_contiguous() and table.numel() >= (rank + 1) * stride
        _check(self.lib, self.lib.mc33hip_bases_from_table(self.ctx, C.c_void_p(table.data_ptr()), int(stride), int(rank), int(bool(concatenated))))

    def emit_at_device_bases(self, V, N, T):
        """emit_into with the id base / output rows that bases_from_table left on the device."""
        _check(self.lib, self.lib.mc33hip_emit_at_device_bases(self.ctx, C.c_void_p(V.data_ptr()), C.c_void_p(N.data_ptr()),
                                                              C.c_void_p(T.data_ptr()), V.shape[0], T.shape[0]))

    def count_finish(self):
        """Waits for what count_async (and the emit behind it) enqueued: (Counts, True), or (Counts, False) when the work
        records or the output buffers were too small - room for the records has been made, repeat the step with count()."""
        cnt = Counts()
        rc = self.lib.mc33hip_count_finish(self.ctx, C.byref(cnt))
        _check(self.lib, rc, allow=(ECAPACITY,))
        return cnt, rc == OK

    # -- a second scalar grid sampled at the vertices (mc33_hip.h: property grid) ------------------------------------------------
    def attach_property(self, tensor, plane0=None):
        """A device tensor [z, y, x] of the grid's dtype, adopted in place: the property grid, as many points per row and rows
        per plane as the grid; its planes are global planes [plane0, plane0 + z) (default: the grid's own plane0)."""
        assert tensor.is_cuda and tensor.dim() == 3 and tensor.stride(2) == 1, "need a device tensor [z, y, x]"
        assert tensor.dtype == self.tensor.dtype and tensor.device == self.device, "the property grid has the grid's dtype and device"
        assert tensor.shape[1] == self.desc.npy and tensor.shape[2] >= self.desc.npx
        _assert_readable(tensor, self.desc.npx, False)  # (the property grid is read at grid points only)
        _check(self.lib, self.lib.mc33hip_property_adopt_device(self.ctx, C.c_void_p(tensor.data_ptr()), tensor.stride(1), tensor.stride(0),
                                                                self.desc.plane0 if plane0 is None else int(plane0), tensor.shape[0]))
        self.property = tensor  # keeps the memory alive

    def detach_property(self):
        _check(self.lib, self.lib.mc33hip_property_drop(self.ctx))
        self.property = None

    def _vertex_rows(self, V):
        import torch
        assert V.is_cuda and V.dim() == 2 and V.shape[1] == 3 and V.is_contiguous()
        assert V.dtype == (torch.float64 if self.dtype == "f64" else torch.float32), "V as extract() returns it"

    def sample_property(self, V):
        """The property grid interpolated at the vertices V [n, 3] (device, as extract() returns them): a float32 tensor [n].
        Raises MC33Error(ERUNTIME) when a vertex needs a plane outside the attached window."""
        import torch
        self._vertex_rows(V)
        out = torch.empty((V.shape[0],), dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.mc33hip_sample_property(self.ctx, C.c_void_p(V.data_ptr()), V.shape[0], C.c_void_p(out.data_ptr())))
        _check(self.lib, self.lib.mc33hip_synchronize(self.ctx))
        return out

    def color_vertices(self, V, palette, lo, hi, nan_color=0xff5c5c5c - (1 << 32)):
        """sample_property mapped through 2..256 palette words (0xAABBGGRR as int32) over the value range [lo, hi]: an int32
        tensor [n]; nan_color (default: the library's DefaultColorMC grey) where the value is NaN."""
        import torch
        self._vertex_rows(V)
        pal = (C.c_int * len(palette))(*[((int(x) + (1 << 31)) % (1 << 32)) - (1 << 31) for x in palette])
        out = torch.empty((V.shape[0],), dtype=torch.int32, device=self.device)
        _check(self.lib, self.lib.mc33hip_color_vertices(self.ctx, C.c_void_p(V.data_ptr()), V.shape[0], pal, len(palette), C.c_double(lo),
                                                         C.c_double(hi), int(nan_color), C.c_void_p(out.data_ptr())))
        _check(self.lib, self.lib.mc33hip_synchronize(self.ctx))
        return out

    # -- curvature of the level set at the vertices, from the resident grid (mc33_hip.h: mc33hip_curvature_vertices) -------------------
    def curvature(self, V, sign=1, which=CURVATURES):
        """Mean, Gaussian and principal curvatures of the grid's level set through the vertices V [n, 3] (device, as extract()
        returns them): a VertexCurvature with a float32 tensor [n] for every name in `which` and the summary of all four.  sign
        +1: a blob of high samples is convex and has mean > 0; -1 the opposite.  Raises MC33Error(EINVAL) for a z-slab or
        inclined context, an axis with fewer than 2 cells, a sign other than +-1."""
        import torch
        self._vertex_rows(V)
        unknown = [k for k in which if k not in CURVATURES]
        if unknown:
            raise ValueError("which: names among %r, not %r" % (CURVATURES, unknown))
        tensors = {k: torch.empty((V.shape[0],), dtype=torch.float32, device=self.device) for k in which}
        a = Curvature()
        a.dV, a.nV, a.sign = V.data_ptr(), V.shape[0], int(sign)
        for k, member in zip(CURVATURES, ("oMean", "oGauss", "oK1", "oK2")):
            setattr(a, member, tensors[k].data_ptr() if k in tensors else None)
        _check(self.lib, self.lib.mc33hip_curvature_vertices(self.ctx, C.byref(a)))
        return VertexCurvature(a, tensors)

    def color_values(self, P, palette, lo, hi, nan_color=0xff5c5c5c - (1 << 32)):
        """The colour step of color_vertices over any float32 device tensor P [n] - what sample_property or curvature returned:
        an int32 tensor [n].  Needs no property grid."""
        import torch
        assert P.is_cuda and P.dim() == 1 and P.dtype == torch.float32 and P.is_contiguous()
        pal = (C.c_int * len(palette))(*[((int(x) + (1 << 31)) % (1 << 32)) - (1 << 31) for x in palette])
        out = torch.empty((P.shape[0],), dtype=torch.int32, device=self.device)
        _check(self.lib, self.lib.mc33hip_color_values(self.ctx, C.c_void_p(P.data_ptr()), P.shape[0], pal, len(palette), C.c_double(lo),
                                                       C.c_double(hi), int(nan_color), C.c_void_p(out.data_ptr())))
        _check(self.lib, self.lib.mc33hip_synchronize(self.ctx))
        return out

    def _extract_rows(self, iso, rng):
        """count, outputs of the counted sizes (one row at least) from torch, emit - enqueued only: (V, N, T, Counts)"""
        import torch
        cnt = self.count(iso, rng or self.full_range())
        V = torch.empty((max(cnt.nV, 1), 3), dtype=torch.float64 if self.dtype == "f64" else torch.float32, device=self.device)
        N = torch.empty((max(cnt.nV, 1), 3), dtype=torch.float32, device=self.device)
        T = torch.empty((max(cnt.nT, 1), 3), dtype=torch.int32, device=self.device)
        _check(self.lib, self.lib.mc33hip_emit(self.ctx, C.c_void_p(V.data_ptr()), C.c_void_p(N.data_ptr()),
                                               C.c_void_p(T.data_ptr()), V.shape[0], T.shape[0]))
        return V, N, T, cnt

    def extract(self, iso, rng=None, with_property=False):
        """Count, allocate exact-size outputs with torch, emit.  Returns (V, N, T, Counts); with_property: and the attached
        property grid's value at every vertex as a fifth element."""
        V, N, T, cnt = self._extract_rows(iso, rng)
        if with_property:
            return V[:cnt.nV], N[:cnt.nV], T[:cnt.nT], cnt, self.sample_property(V[:cnt.nV])
        self.stream.synchronize()
        return V[:cnt.nV], N[:cnt.nV], T[:cnt.nT], cnt

    # -- measures of a finished mesh, taken on the device (mc33_hip.h: mc33hip_measure_surface and its siblings) ------------------
    def _triangle_rows(self, T):
        import torch
        assert T.is_cuda and T.dim() == 2 and T.shape[1] == 3 and T.is_contiguous() and T.dtype == torch.int32, "T as extract() returns it"

    def measure(self, V, T, P=None):
        """Area, signed volume, first moments, bounding box of the mesh V [n, 3], T [m, 3] (device tensors, as extract() returns
        them) and, with P (float32 [n], what sample_property returned), the integral of P over the surface: a SurfaceMeasures.
        Raises MC33Error(ERUNTIME) when a triangle names a vertex >= n."""
        import torch
        self._vertex_rows(V)
        self._triangle_rows(T)
        if P is not None:
            assert P.is_cuda and P.dtype == torch.float32 and P.is_contiguous() and P.numel() == V.shape[0]
        m = Measures()
        _check(self.lib, self.lib.mc33hip_measure_surface(self.ctx, C.c_void_p(V.data_ptr()), V.shape[0], C.c_void_p(T.data_ptr()), T.shape[0],
                                                          C.c_void_p(P.data_ptr()) if P is not None else None, C.byref(m)))
        return SurfaceMeasures(m)

    def label_components(self, T, nV):
        """(labels, components, unreferenced): labels an int32 tensor [nV] holding the uint32 words label[v] = the smallest
        vertex index connected to v through triangles of T."""
        import torch
        self._triangle_rows(T)
        labels = torch.empty((int(nV),), dtype=torch.int32, device=self.device)
        nc, nu = C.c_ulonglong(), C.c_ulonglong()
        _check(self.lib, self.lib.mc33hip_label_components(self.ctx, C.c_void_p(T.data_ptr()), T.shape[0], int(nV), C.c_void_p(labels.data_ptr()),
                                                           C.byref(nc), C.byref(nu)))
        return labels, nc.value, nu.value

    def measure_components(self, V, T, labels=None):
        """The component table - root, nV, nT, area, volume per component, in ascending order of root - as a numpy structured
        array; labels: what label_components returned for T (made here when None)."""
        self._vertex_rows(V)
        self._triangle_rows(T)
        if labels is None:
            labels = self.label_components(T, V.shape[0])[0]
        assert labels.is_cuda and labels.is_contiguous() and labels.numel() == V.shape[0] and labels.element_size() == 4
        return self._component_table(self.lib.mc33hip_measure_components, Component,
                                     C.c_void_p(V.data_ptr()), V.shape[0], C.c_void_p(T.data_ptr()), T.shape[0], C.c_void_p(labels.data_ptr()))

    def _component_table(self, fn, row, *args):
        """fn(ctx, *args, table, capacity, &n) twice: without a table for the number of rows, then into a numpy array of them"""
        import numpy as np
        n = C.c_ulonglong()
        _check(self.lib, fn(self.ctx, *args, None, 0, C.byref(n)), allow=(ECAPACITY,))
        table = np.zeros(n.value, dtype=np.dtype(row))
        if n.value:
            _check(self.lib, fn(self.ctx, *args, C.c_void_p(table.ctypes.data), n.value, C.byref(n)))
        return table

    def measure_iso(self, iso, rng=None, with_property=False):
        """Count, emit into torch tensors, measure - nothing but the result crosses the link; with_property: the attached
        property grid is sampled at the vertices first and its integral over the surface filled in."""
        import torch
        V, N, T, cnt = self._extract_rows(iso, rng)
        P = None
        if with_property:
            P = torch.empty((max(cnt.nV, 1),), dtype=torch.float32, device=self.device)
            _check(self.lib, self.lib.mc33hip_sample_property(self.ctx, C.c_void_p(V.data_ptr()), cnt.nV, C.c_void_p(P.data_ptr())))
        m = Measures()
        _check(self.lib, self.lib.mc33hip_measure_surface(self.ctx, C.c_void_p(V.data_ptr()), cnt.nV, C.c_void_p(T.data_ptr()), cnt.nT,
                                                          C.c_void_p(P.data_ptr()) if P is not None else None, C.byref(m)))
        return SurfaceMeasures(m)

    # -- topology of a finished triangle list, taken on the device (mc33_hip.h: mc33hip_surface_topology) --------------------------
    def topology(self, T, nV):
        """Edges, boundary / non-manifold / misoriented edges, degenerate triangles, boundary loops, Euler number, components and
        genus of the triangle list T [m, 3] over nV vertices: a SurfaceTopology.  Raises MC33Error(ERUNTIME) when a triangle
        names a vertex >= nV."""
        self._triangle_rows(T)
        t = Topology()
        _check(self.lib, self.lib.mc33hip_surface_topology(self.ctx, C.c_void_p(T.data_ptr()), T.shape[0], int(nV), C.byref(t)))
        return SurfaceTopology(t)

    def component_topology(self, T, nV, labels=None):
        """The same counts per component, with euler and genus (-1: not defined) - the rows of measure_components, in ascending
        order of root - as a numpy structured array; labels: what label_components returned for T (made here when None)."""
        self._triangle_rows(T)
        if labels is None:
            labels = self.label_components(T, nV)[0]
        assert labels.is_cuda and labels.is_contiguous() and labels.numel() == int(nV) and labels.element_size() == 4
        return self._component_table(self.lib.mc33hip_component_topology, ComponentTopology,
                                     C.c_void_p(T.data_ptr()), T.shape[0], int(nV), C.c_void_p(labels.data_ptr()))

    def topology_iso(self, iso, rng=None):
        """Count, emit into torch tensors, topology - nothing but the result crosses the link."""
        V, N, T, cnt = self._extract_rows(iso, rng)
        t = Topology()
        _check(self.lib, self.lib.mc33hip_surface_topology(self.ctx, C.c_void_p(T.data_ptr()), cnt.nT, cnt.nV, C.byref(t)))
        return SurfaceTopology(t)

    # -- keep or drop components of a finished mesh, on the device (mc33_hip.h: mc33hip_compact_components) ------------------------
    def select_components(self, table, topo_table=None, **criteria):
        """The roots of the rows of `table` (measure_components) that pass the criteria - min_triangles, min_area, min_abs_volume,
        largest, closed_only (needs topo_table: component_topology) - ascending, as a numpy uint32 array.  The rule is the
        library's MC33_select_components (include/marching_cubes_33.h): there is no second implementation."""
        import numpy as np
        f = ComponentFilter(**criteria)
        table = np.ascontiguousarray(table, dtype=np.dtype(Component))
        if topo_table is not None:
            topo_table = np.ascontiguousarray(topo_table, dtype=np.dtype(ComponentTopology))
            assert topo_table.shape[0] == table.shape[0]
        roots = np.zeros(max(table.shape[0], 1), np.uint32)
        n = self.lib.MC33_select_components(C.c_void_p(table.ctypes.data) if table.shape[0] else None,
                                            C.c_void_p(topo_table.ctypes.data) if topo_table is not None else None, table.shape[0], C.byref(f),
                                            C.c_void_p(roots.ctypes.data))
        if n < 0:
            raise ValueError("MC33_select_components refused its arguments (closed_only needs topo_table)")
        return roots[:n].copy()

    def _attribute_words(self, attrs, nV):
        """attrs as a tuple, each asserted to be a contiguous device tensor of one 4-byte word per vertex"""
        attrs = tuple(attrs)
        for x in attrs:
            assert x.is_cuda and x.is_contiguous() and x.numel() == nV and x.element_size() == 4, "an attribute is one 4-byte word per vertex"
        return attrs

    def _into_new_rows(self, fn, a, normals, vdtype, attrs):
        """A mesh pass with outputs of its own (fn: the library's function, a: its argument struct with the inputs filled in): the
        size query - null outputs, which the library refuses for room -, exact-size outputs from torch (one row at least), the
        call proper.  Returns (V2, N2, T2, attrs2, vmap) cut to a.nV_out / a.nT_out rows; N2 None unless `normals`."""
        import torch
        _check(self.lib, fn(self.ctx, C.byref(a)), allow=(ECAPACITY,))
        nV, nV2, nT2 = int(a.nV), int(a.nV_out), int(a.nT_out)
        V2 = torch.empty((max(nV2, 1), 3), dtype=vdtype, device=self.device)
        N2 = torch.empty((max(nV2, 1), 3), dtype=torch.float32, device=self.device) if normals else None
        T2 = torch.empty((max(nT2, 1), 3), dtype=torch.int32, device=self.device)
        attrs2 = [torch.empty((max(nV2, 1),), dtype=x.dtype, device=self.device) for x in attrs]
        vmap = torch.empty((max(nV, 1),), dtype=torch.int32, device=self.device)
        a.oV, a.oT, a.oN, a.oMap, a.capV, a.capT = V2.data_ptr(), T2.data_ptr(), (N2.data_ptr() if normals else None), vmap.data_ptr(), nV2, nT2
        for k, x in enumerate(attrs2):
            a.oAttr[k] = x.data_ptr()
        _check(self.lib, fn(self.ctx, C.byref(a)))
        return V2[:nV2], (N2[:nV2] if normals else None), T2[:nT2], [x[:nV2] for x in attrs2], vmap[:nV]

    def compact_components(self, V, N, T, labels, roots, invert=False, attrs=()):
        """Keeps the components of the mesh V, N, T (device tensors, as extract() returns them) whose root is in `roots` - or, with
        invert, all others - and drops every vertex no triangle names: (V2, N2, T2, attrs2, vmap, components_kept), exact-size
        device tensors in the order of the input, T2 renumbered; attrs: up to two device tensors of one 4-byte word per vertex,
        compacted alongside; vmap (int32 [nV], the uint32 words new[v], 0xFFFFFFFF where v was dropped) carries further arrays.
        labels: what label_components returned for T."""
        import numpy as np
        import torch
        self._vertex_rows(V)
        self._triangle_rows(T)
        nV = V.shape[0]
        assert N.is_cuda and N.is_contiguous() and N.dtype == torch.float32 and tuple(N.shape) == (nV, 3)
        assert labels.is_cuda and labels.is_contiguous() and labels.numel() == nV and labels.element_size() == 4
        attrs = self._attribute_words(attrs, nV)
        roots = np.ascontiguousarray(np.asarray(roots).reshape(-1), dtype=np.uint32)
        a = Compaction()
        a.V, a.N, a.T, a.label, a.nV, a.nT = V.data_ptr(), N.data_ptr(), T.data_ptr(), labels.data_ptr(), nV, T.shape[0]
        for k, x in enumerate(attrs[:2]):
            a.attr[k] = x.data_ptr()
        a.n_attr, a.invert = len(attrs), int(bool(invert))
        a.roots, a.n_roots = (roots.ctypes.data if roots.size else None), roots.size
        return self._into_new_rows(self.lib.mc33hip_compact_components, a, True, V.dtype, attrs) + (int(a.components_kept),)

    def extract_filtered(self, iso, rng=None, with_property=False, **criteria):
        """extract, label, measure (and component_topology, only for closed_only), select_components(**criteria), compact - the
        whole surface never leaves the device.  Returns (V, N, T, kept, dropped) - components kept and dropped - and, with
        with_property, the attached property grid's value at the kept vertices as a sixth element."""
        got = self.extract(iso, rng, with_property)
        V, N, T = got[0], got[1], got[2]
        labels = self.label_components(T, V.shape[0])[0]
        table = self.measure_components(V, T, labels)
        topo = self.component_topology(T, V.shape[0], labels) if criteria.get("closed_only") else None
        roots = self.select_components(table, topo, **criteria)
        V2, N2, T2, attrs2, _, kept = self.compact_components(V, N, T, labels, roots, attrs=(got[4],) if with_property else ())
        out = (V2, N2, T2, kept, table.shape[0] - kept)
        return out + (attrs2[0],) if with_property else out

    # -- smooth a finished mesh on the device (mc33_hip.h: mc33hip_smooth_surface) -------------------------------------------------
    def smooth(self, V, T, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, normals=True, out=None):
        """Taubin's lambda | mu smoothing of the mesh V [n, 3], T [m, 3] (device tensors, as extract() returns them): `iterations`
        times a pass with factor lam, then one with mu; pin_boundary leaves the vertices of open edges where they are.  Returns
        (V2, N2, info): the smoothed vertices - in `out` when given, which may be V itself (in place) -, the normals recomputed
        from them (None with normals=False) and a dict of max_degree, isolated_vertices, boundary_vertices, invalid_triangles.
        T is not changed.  Raises MC33Error(ERUNTIME) when a triangle names a vertex >= n (the outputs are complete without it)."""
        import torch
        self._vertex_rows(V)
        self._triangle_rows(T)
        nV = V.shape[0]
        if out is None:
            out = torch.empty_like(V)
        self._vertex_rows(out)
        assert out.dtype == V.dtype and out.shape[0] == nV and out.device == V.device
        N2 = torch.empty((nV, 3), dtype=torch.float32, device=self.device) if normals else None
        a = Smoothing()
        a.V, a.T, a.nV, a.nT = V.data_ptr(), T.data_ptr(), nV, T.shape[0]
        a.iterations, a.lam, a.mu, a.pin_boundary = int(iterations), float(lam), float(mu), int(bool(pin_boundary))
        a.oV, a.oN = out.data_ptr(), (N2.data_ptr() if normals else None)
        _check(self.lib, self.lib.mc33hip_smooth_surface(self.ctx, C.byref(a)))
        return out, N2, {k: int(getattr(a, k)) for k in ("max_degree", "isolated_vertices", "boundary_vertices", "invalid_triangles")}

    def vertex_normals(self, V, T):
        """Normals of the mesh V, T recomputed from its triangles - per vertex the sum of the cross products of the triangles
        that name it, normalised; the stored winding decides the sign: a float32 tensor [n, 3]."""
        import torch
        self._vertex_rows(V)
        self._triangle_rows(T)
        N2 = torch.empty((V.shape[0], 3), dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.mc33hip_vertex_normals(self.ctx, C.c_void_p(V.data_ptr()), V.shape[0], C.c_void_p(T.data_ptr()), T.shape[0],
                                                         C.c_void_p(N2.data_ptr())))
        return N2

    def extract_smoothed(self, iso, rng=None, with_property=False, error=False, **smoothing):
        """extract, then smooth(**smoothing) in place - the surface never leaves the device.  Returns (V, N, T, Counts) with the
        smoothed vertices and their recomputed normals (the extracted N with normals=False) and, with with_property, the attached
        property grid's value at the UNSMOOTHED vertices as a fifth element.  error=True: a dict `info` behind the Counts whose
        "error" is surface_distance(smoothed, extracted) - how far the passes moved the surface; the extracted vertices are kept
        in a second tensor for it."""
        got = self.extract(iso, rng, with_property)
        V, N, T, cnt = got[:4]
        V0 = V.clone() if error else None
        V2, N2, _ = self.smooth(V, T, out=V, **smoothing)
        out = (V2, N2 if N2 is not None else N, T, cnt)
        if error:
            out = out + ({"error": self.surface_distance(V2, T, V0, T)},)
        return out + (got[4],) if with_property else out

    def smooth_timing(self):
        """hipEvent times of the last smooth / vertex_normals after set_timing(2): (adjacency ms, normals ms, [ms per pass])."""
        adj, nrm, n = C.c_float(), C.c_float(), C.c_uint()
        ms = (C.c_float * 64)()
        _check(self.lib, self.lib.mc33hip_smooth_timing(self.ctx, C.byref(adj), C.byref(nrm), ms, 64, C.byref(n)))
        return adj.value, nrm.value, [ms[k] for k in range(n.value)]

    # -- simplify a finished mesh on the device (mc33_hip.h: mc33hip_simplify_surface) ---------------------------------------------
    def simplify(self, V, T, cell, origin=None, mode="mean", drop_duplicates=True, normals=True, attrs=()):
        """Vertex clustering of the mesh V [n, 3], T [m, 3] (device tensors, as extract() returns them) on the lattice of cells
        `cell` (a number or three, world units) wide from `origin` (default: the grid's r0): the vertices of a cell become their
        mean (mode "mean") or the first of them ("first"), triangles that lose a corner go and, with drop_duplicates, so do
        repeated ones.  Returns (V2, N2, T2, attrs2, vmap, info): exact-size device tensors - N2 the normals recomputed from the
        output (None with normals=False); attrs: up to two device tensors of one 4-byte word per vertex, the word of a cell's first
        vertex is kept; vmap int32 [n], the uint32 words of the new index, 0xFFFFFFFF where the vertex left - and a dict of the
        call's counts and `ratio`, output over input triangles.  Raises MC33Error(ERUNTIME) when a triangle names a vertex >= n."""
        self._vertex_rows(V)
        self._triangle_rows(T)
        nV = V.shape[0]
        attrs = self._attribute_words(attrs, nV)
        cell = (float(cell),) * 3 if not hasattr(cell, "__len__") else tuple(float(x) for x in cell)
        origin = tuple(self.desc.r0) if origin is None else tuple(float(x) for x in origin)
        a = Simplification()
        a.V, a.T, a.nV, a.nT = V.data_ptr(), T.data_ptr(), nV, T.shape[0]
        for k, x in enumerate(attrs[:2]):
            a.attr[k] = x.data_ptr()
        a.n_attr = len(attrs)
        a.origin, a.cell = (C.c_double * 3)(*origin), (C.c_double * 3)(*cell)
        a.mode, a.drop_duplicates = SIMPLIFY_MODES[mode], int(bool(drop_duplicates))
        out = self._into_new_rows(self.lib.mc33hip_simplify_surface, a, normals, V.dtype, attrs)
        info = {n: int(getattr(a, n)) for n in ("nV_out", "nT_out", "clusters", "max_cluster", "collapsed_triangles", "duplicate_triangles",
                                                "invalid_triangles", "clamped_vertices")}
        info["ratio"] = info["nT_out"] / T.shape[0] if T.shape[0] else 0.0
        return out + (info,)

    def extract_simplified(self, iso, cell_in_grid_cells, rng=None, with_property=False, error=False, **kw):
        """extract, then simplify on the lattice of the grid - origin r0, cells of cell_in_grid_cells (a number or three) grid
        spacings - the whole surface never leaves the device.  Returns (V, N, T, info) and, with with_property, the attached
        property grid's value at the first vertex of every kept cell as a fifth element.  **kw: mode, drop_duplicates.
        error=True: info["error"] is surface_distance(simplified, extracted) - what the clustering gave away, both directions."""
        got = self.extract(iso, rng, with_property)
        c = (float(cell_in_grid_cells),) * 3 if not hasattr(cell_in_grid_cells, "__len__") else tuple(float(x) for x in cell_in_grid_cells)
        cell = tuple(c[k] * self.desc.d[k] for k in range(3))
        V2, N2, T2, attrs2, _, info = self.simplify(got[0], got[2], cell, attrs=(got[4],) if with_property else (), **kw)
        if error:
            info["error"] = self.surface_distance(V2, T2, got[0], got[2])
        out = (V2, N2, T2, info)
        return out + (attrs2[0],) if with_property else out

    # -- clip a finished mesh by a plane on the device (mc33_hip.h: mc33hip_clip_surface) ------------------------------------------
    def clip(self, V, N, T, plane, attrs=(), attr_modes=()):
        """The mesh V [n, 3], N [n, 3] (or None), T [m, 3] (device tensors, as extract() returns them) cut by the plane
        (a, b, c, w): the half space a x + b y + c z + w >= 0 stays, triangles the plane crosses are cut, the new vertices are
        shared.  Returns (V2, N2, T2, attrs2, vmap, info): exact-size device tensors - N2 None without N; attrs: up to two device
        tensors of one 4-byte word per vertex, attr_modes "copy" (a new vertex takes the word of its end inside; the default) or
        "lerp_f32" (the words are floats and are interpolated); vmap int32 [n], the uint32 words of the new index of a kept vertex,
        0xFFFFFFFF where it left - and a dict of the call's ten counts.  Raises MC33Error(ERUNTIME) when a triangle names a
        vertex >= n (the outputs are complete without it)."""
        import torch
        self._vertex_rows(V)
        self._triangle_rows(T)
        nV = V.shape[0]
        if N is not None:
            assert N.is_cuda and N.is_contiguous() and N.dtype == torch.float32 and tuple(N.shape) == (nV, 3)
        attrs = self._attribute_words(attrs, nV)
        modes = [CLIP_MODES[m] if isinstance(m, str) else int(m) for m in attr_modes] + [0] * (len(attrs) - len(attr_modes))
        a = Clipping()
        a.V, a.N, a.T, a.nV, a.nT = V.data_ptr(), (N.data_ptr() if N is not None else None), T.data_ptr(), nV, T.shape[0]
        for k, x in enumerate(attrs[:2]):
            a.attr[k], a.attr_mode[k] = x.data_ptr(), modes[k]
        a.n_attr = len(attrs)
        a.plane = (C.c_double * 4)(*[float(x) for x in plane])
        out = self._into_new_rows(self.lib.mc33hip_clip_surface, a, N is not None, V.dtype, attrs)
        return out + ({n: int(getattr(a, n)) for n in CLIP_COUNTS},)

    def extract_clipped(self, iso, planes, rng=None, with_property=False):
        """extract, then clip by every plane of `planes` (4-tuples a, b, c, w; clip_box(lo, hi) makes the six of a box) one after
        another - the whole surface never leaves the device.  Returns (V, N, T, infos) - infos: the dict of every clip - and,
        with with_property, the attached property grid's value at the FINAL vertices as a fifth element: a new vertex gets the
        value of its own position."""
        got = self.extract(iso, rng)
        V, N, T = got[0], got[1], got[2]
        infos = []
        for plane in planes:
            V, N, T, _, _, info = self.clip(V, N, T, plane)
            infos.append(info)
        out = (V, N, T, infos)
        return out + (self.sample_property(V),) if with_property else out

    # -- close a finished mesh at the faces of a box of grid points (mc33_hip.h: mc33hip_cap_surface) ---------------------------------
    def cap(self, V, N, T, iso, box=None, invert=False, attrs=()):
        """The mesh V [n, 3], N [n, 3], T [m, 3] (device tensors, as extract() of `iso` returns them) closed at the six faces of
        `box` = (lo, hi) in grid points - None: the whole grid; the z bounds of the range for a z-range extraction: new vertices at
        the solid grid points of the faces, new triangles joined to the surface's rim by its own vertex ids.  invert: cap the
        other side - the triangles come back with their second and third index exchanged, the normals negated.  attrs: up to two
        device tensors of one 4-byte word per vertex; a new vertex gets NaN in a float32 tensor, 0 in any other.  Returns (V2, N2,
        T2, attrs2, info): NEW exact-size device tensors whose first n / m rows are the input's (the input is left alone), and a dict
        of the call's counts - closed: 1 when nothing was skipped.  Raises MC33Error(ERUNTIME) when a triangle names a vertex >= n
        (the outputs are complete without it)."""
        import torch
        self._vertex_rows(V)
        self._triangle_rows(T)
        nV, nT = V.shape[0], T.shape[0]
        assert N.is_cuda and N.is_contiguous() and N.dtype == torch.float32 and tuple(N.shape) == (nV, 3)
        attrs = self._attribute_words(attrs, nV)
        lo, hi = box if box is not None else ((0, 0, 0), (self.desc.npx - 1, self.desc.npy - 1, self.desc.nz_total))
        a = Capping()
        a.V, a.N, a.T, a.nV, a.nT = V.data_ptr(), N.data_ptr(), T.data_ptr(), nV, nT
        a.iso, a.invert = float(iso), int(bool(invert))
        a.lo, a.hi = (C.c_uint * 3)(*[int(x) for x in lo]), (C.c_uint * 3)(*[int(x) for x in hi])
        for k, x in enumerate(attrs[:2]):
            a.attr[k], a.attr_mode[k] = x.data_ptr(), (1 if x.dtype == torch.float32 else 0)
        a.n_attr = len(attrs)
        _check(self.lib, self.lib.mc33hip_cap_surface(self.ctx, C.byref(a)), allow=(ECAPACITY,))  # the size query: no room, nothing is written
        nV2, nT2 = int(a.nV_out), int(a.nT_out)
        V2 = torch.empty((max(nV2, 1), 3), dtype=V.dtype, device=self.device)
        N2 = torch.empty((max(nV2, 1), 3), dtype=torch.float32, device=self.device)
        T2 = torch.empty((max(nT2, 1), 3), dtype=torch.int32, device=self.device)
        attrs2 = [torch.empty((max(nV2, 1),), dtype=x.dtype, device=self.device) for x in attrs]
        V2[:nV].copy_(V)
        N2[:nV].copy_(N)
        T2[:nT].copy_(T)
        for x2, x in zip(attrs2, attrs):
            x2[:nV].copy_(x)
        a.V, a.N, a.T, a.capV, a.capT = V2.data_ptr(), N2.data_ptr(), T2.data_ptr(), V2.shape[0], T2.shape[0]
        for k, x in enumerate(attrs2):
            a.attr[k] = x.data_ptr()
        _check(self.lib, self.lib.mc33hip_cap_surface(self.ctx, C.byref(a)))
        return V2[:nV2], N2[:nV2], T2[:nT2], [x[:nV2] for x in attrs2], {n: int(getattr(a, n)) for n in CAP_COUNTS}

    def extract_capped(self, iso, rng=None, invert=False, with_property=False):
        """extract, then close the surface at the faces of the grid - of the planes z_begin .. z_end of rng, where one is given, whose
        surface is extracted on its own - on the device.
        Returns (V, N, T, info) - what measure, topology, smooth, simplify, clip and section take - and, with with_property, the
        attached property grid's value at the FINAL vertices as a fifth element: a new vertex gets the value of its own position."""
        if rng is None or (rng.z_begin == 0 and rng.z_end == self.desc.nz_total):
            got, box = self.extract(iso), None
        else:
            # A z range of this context is a slab's piece: its triangles name vertices of the slice below.  The surface of the planes
            # z_begin .. z_end alone comes from a context on those planes of the same tensor; the caps need the whole grid, here.
            assert self.desc.plane0 == 0 and rng.z_begin < rng.z_end <= self.desc.nz_total, "a z range of a whole grid"
            r0, d = tuple(self.desc.r0), tuple(self.desc.d)
            sub = DeviceGrid(self.tensor[rng.z_begin:rng.z_end + 1], r0=(r0[0], r0[1], r0[2] + rng.z_begin * d[2]), d=d, npx=self.desc.npx, volatile=True)
            try:
                got = sub.extract(iso)
            finally:
                sub.close()
            box = ((0, 0, rng.z_begin), (self.desc.npx - 1, self.desc.npy - 1, rng.z_end))
        V, N, T, _, info = self.cap(got[0], got[1], got[2], iso, box, invert)
        out = (V, N, T, info)
        return out + (self.sample_property(V),) if with_property else out

    # -- draw a finished mesh on the device (mc33_hip.h: mc33hip_render_surface) ---------------------------------------------------------
    def render(self, V, N, T, colors, view, want=IMAGE_RGBA | IMAGE_DEPTH | IMAGE_IDS, base_color=0xff5c5c5c):
        """The mesh V [n, 3], N [n, 3], T [m, 3] (device tensors, as extract() returns them) drawn as `view` (a View: matrix, image
        size, cull, two_sided, light, ambient, diffuse, background) sees it.  colors: an int32 device tensor [n] of words 0xAABBGGRR
        (what color_vertices returns), or None: base_color for every vertex.  want: IMAGE_RGBA | IMAGE_DEPTH | IMAGE_IDS; 0 asks for
        the counts alone.  Returns (rgba, depth, ids, info): device tensors [height, width] - int32 words, float32 with +inf where
        nothing was drawn, int32 triangle indices with -1 there -, None for an array not wanted, and a dict of the call's counts.
        Raises MC33Error(ERUNTIME) when a triangle names a vertex >= n (the image is complete without it)."""
        import torch
        self._vertex_rows(V)
        self._triangle_rows(T)
        nV, nT = V.shape[0], T.shape[0]
        assert N.is_cuda and N.is_contiguous() and N.dtype == torch.float32 and tuple(N.shape) == (nV, 3)
        if colors is not None:
            (colors,) = self._attribute_words((colors,), nV)
        a = Rendering()
        a.V, a.N, a.T, a.nV, a.nT = V.data_ptr(), N.data_ptr(), T.data_ptr(), nV, nT
        a.C = colors.data_ptr() if colors is not None and nV else None
        a.m, a.light = view.m, view.light
        a.width, a.height, a.cull, a.two_sided = view.width, view.height, view.cull, view.two_sided
        a.ambient, a.diffuse, a.background, a.base_color = view.ambient, view.diffuse, view.background, int(base_color) & 0xFFFFFFFF
        shape = (max(int(view.height), 1), max(int(view.width), 1))
        rgba = torch.empty(shape, dtype=torch.int32, device=self.device) if want & IMAGE_RGBA else None
        depth = torch.empty(shape, dtype=torch.float32, device=self.device) if want & IMAGE_DEPTH else None
        ids = torch.empty(shape, dtype=torch.int32, device=self.device) if want & IMAGE_IDS else None
        a.oRGBA, a.oDepth, a.oTri = (x.data_ptr() if x is not None else None for x in (rgba, depth, ids))
        _check(self.lib, self.lib.mc33hip_render_surface(self.ctx, C.byref(a)))
        return rgba, depth, ids, {n: int(getattr(a, n)) for n in RENDER_COUNTS}

    def extract_rendered(self, iso, view, want=IMAGE_RGBA | IMAGE_DEPTH | IMAGE_IDS, colors=None):
        """extract, then draw the surface on the device: (rgba, depth, ids, info) as render() returns them, info with the surface's
        nV and nT.  colors(V) -> an int32 tensor of colour words for the vertices (color_vertices, say), or None."""
        V, N, T, cnt = self.extract(iso)
        rgba, depth, ids, info = self.render(V, N, T, colors(V) if colors is not None else None, view, want)
        info["nV"], info["nT"] = int(cnt.nV), int(cnt.nT)
        return rgba, depth, ids, info

    # -- distance between surfaces on the device (mc33_hip.h: mc33hip_surface_distance) --------------------------------------------------
    def distance(self, P, V, T, signed=False, nearest_point=False):
        """For every point of P [p, 3] the nearest point of the mesh V [n, 3], T [m, 3] (device tensors, P and V of one dtype, as
        extract() returns them).  Returns (dist, tri, point, info): dist float32 [p] - with signed=True negative behind the plane
        of the nearest triangle, which near an edge is only as good as that plane -, tri int32 [p], the uint32 words of the nearest
        triangle's index, point [p, 3] the nearest point itself (None without nearest_point), and a dict of the call's summary over
        the matched points: matched_points, unmatched_points, invalid_triangles, nonfinite_triangles, max, min, argmax, argmin, sum,
        sum_sq, mean, rms, and the search's own lattice and triangle_tests.  A point without a winner - not finite, or no usable
        triangle - has +inf, -1 and NaN.  Raises MC33Error(ERUNTIME) when a triangle names a vertex >= n (the outputs are complete
        without it)."""
        import torch
        self._vertex_rows(P)
        self._vertex_rows(V)
        self._triangle_rows(T)
        assert P.dtype == V.dtype
        nP = P.shape[0]
        dist = torch.empty((max(nP, 1),), dtype=torch.float32, device=self.device)
        tri = torch.empty((max(nP, 1),), dtype=torch.int32, device=self.device)
        point = torch.empty((max(nP, 1), 3), dtype=P.dtype, device=self.device) if nearest_point else None
        a = Distance()
        a.P, a.nP, a.V, a.T, a.nV, a.nT = P.data_ptr(), nP, V.data_ptr(), T.data_ptr(), V.shape[0], T.shape[0]
        a.signed_distance = int(bool(signed))
        a.oDist, a.oTri, a.oPoint = dist.data_ptr(), tri.data_ptr(), (point.data_ptr() if nearest_point else None)
        _check(self.lib, self.lib.mc33hip_surface_distance(self.ctx, C.byref(a)))
        return dist[:nP], tri[:nP], (point[:nP] if nearest_point else None), self._distance_info(a)

    @staticmethod
    def _distance_info(a):
        info = {n: getattr(a, n) for n in DISTANCE_FIELDS}
        info["lattice"] = tuple(a.lattice)
        m = info["matched_points"]
        info["mean"] = info["sum"] / m if m else 0.0
        info["rms"] = math.sqrt(info["sum_sq"] / m) if m else 0.0
        return info

    def surface_distance(self, V1, T1, V2, T2):
        """How far two meshes are from each other, SAMPLED AT THEIR VERTICES ONLY: the vertices of V1 against the triangles of V2,
        T2 ("forward") and the vertices of V2 against V1, T1 ("backward"), each the info dict of distance(), and "hausdorff", the
        larger of the two max.  The interior of a coarse triangle can be farther from the other surface than any of its corners:
        the figure is a lower bound of the true Hausdorff distance.  T1 itself is only the target of the backward direction:
        vertices no triangle names count as points too."""
        fwd, bwd = self.distance(V1, V2, T2)[3], self.distance(V2, V1, T1)[3]
        return {"forward": fwd, "backward": bwd, "hausdorff": max(fwd["max"], bwd["max"])}

    def distance_timing(self):
        """hipEvent times in ms of the last distance() after set_timing(2): (build, query, reduce)."""
        ms = (C.c_float * 3)()
        _check(self.lib, self.lib.mc33hip_distance_timing(self.ctx, C.byref(ms)))
        return tuple(ms)

    # -- section a finished mesh by planes on the device (mc33_hip.h: mc33hip_section_surface and its siblings) ----------------------
    def section(self, V, T, plane, attrs=(), attr_modes=()):
        """The contour where the plane (a, b, c, w) meets the mesh V [n, 3], T [m, 3] (device tensors, as extract() returns them):
        the boundary clip() opens on the same input, as points and directed segments.  Returns a SectionResult: exact-size
        device tensors P [p, 3], S [s, 2] (int32, the uint32 words of point indices), attrs (attr_modes as for clip), label and
        next (int32 [p]), point_map (int32 [n]), the thirteen counts in .info, and length, area_vector, area (signed: it
        follows the winding, as the volume does), origin.  Raises MC33Error(ERUNTIME) when a triangle names a vertex >= n."""
        import torch
        self._vertex_rows(V)
        self._triangle_rows(T)
        nV = V.shape[0]
        attrs = self._attribute_words(attrs, nV)
        modes = [CLIP_MODES[m] if isinstance(m, str) else int(m) for m in attr_modes] + [0] * (len(attrs) - len(attr_modes))
        a = Sectioning()
        a.V, a.T, a.nV, a.nT = V.data_ptr(), T.data_ptr(), nV, T.shape[0]
        for k, x in enumerate(attrs[:2]):
            a.attr[k], a.attr_mode[k] = x.data_ptr(), modes[k]
        a.n_attr = len(attrs)
        a.plane = (C.c_double * 4)(*[float(x) for x in plane])
        fn = self.lib.mc33hip_section_surface
        _check(self.lib, fn(self.ctx, C.byref(a)), allow=(ECAPACITY,))  # the size query
        nP, nS = int(a.nP_out), int(a.nS_out)
        P = torch.empty((max(nP, 1), 3), dtype=V.dtype, device=self.device)
        S = torch.empty((max(nS, 1), 2), dtype=torch.int32, device=self.device)
        attrs2 = [torch.empty((max(nP, 1),), dtype=x.dtype, device=self.device) for x in attrs]
        label, nxt = (torch.empty((max(nP, 1),), dtype=torch.int32, device=self.device) for _ in range(2))
        pmap = torch.empty((max(nV, 1),), dtype=torch.int32, device=self.device)
        a.oP, a.oS, a.oLabel, a.oNext, a.oPointMap, a.capP, a.capS = P.data_ptr(), S.data_ptr(), label.data_ptr(), nxt.data_ptr(), pmap.data_ptr(), nP, nS
        for k, x in enumerate(attrs2):
            a.oAttr[k] = x.data_ptr()
        _check(self.lib, fn(self.ctx, C.byref(a)))
        return SectionResult(a, P[:nP], S[:nS], [x[:nP] for x in attrs2], label[:nP], nxt[:nP], pmap[:nV])

    def section_contours(self, section):
        """The contour table of a SectionResult - root, points, segments, open_ends, branch_points, closed, length, area per
        contour, in ascending order of root - as a numpy structured array.  length and area are added with atomics on the
        device: their last bits may differ from call to call."""
        plane = (C.c_double * 4)(*section.plane)
        return self._component_table(lambda ctx, *args: self.lib.mc33hip_section_contours(ctx, *args[:5], C.byref(plane), *args[5:]), Contour,
                                     C.c_void_p(section.P.data_ptr()), section.P.shape[0], C.c_void_p(section.S.data_ptr()), section.S.shape[0],
                                     C.c_void_p(section.label.data_ptr()))

    def section_ladder(self, V, T, normal, offsets):
        """What section() reports along a stack of parallel planes (a, b, c, w_k) - up to 255 offsets w_k, strictly ascending -
        in one pass over T and without geometry: (segments uint64 [n], length float64 [n], area float64 [n]) as numpy arrays.
        segments[k] is section()'s nS_out exactly; the doubles are added with atomics."""
        import numpy as np
        self._vertex_rows(V)
        self._triangle_rows(T)
        offsets = [float(x) for x in offsets]
        n = len(offsets)
        w = (C.c_double * max(n, 1))(*offsets)
        seg, length, area = np.zeros(n, np.uint64), np.zeros(n, np.float64), np.zeros(n, np.float64)
        bad = C.c_ulonglong()
        nrm = (C.c_double * 3)(*[float(x) for x in normal])
        _check(self.lib, self.lib.mc33hip_section_ladder(self.ctx, C.c_void_p(V.data_ptr()), V.shape[0], C.c_void_p(T.data_ptr()), T.shape[0], C.byref(nrm),
                                                         C.cast(w, C.POINTER(C.c_double)), min(n, 0xFFFFFFFF),
                                                         seg.ctypes.data_as(C.POINTER(C.c_ulonglong)) if n else None,
                                                         length.ctypes.data_as(C.POINTER(C.c_double)) if n else None,
                                                         area.ctypes.data_as(C.POINTER(C.c_double)) if n else None, C.byref(bad)))
        return seg, length, area

    def extract_section(self, iso, plane, rng=None, with_property=False):
        """extract, then section by the plane - the surface never leaves the device.  Returns the SectionResult and, with
        with_property, the attached property grid's value at the points of the section (each at its own position) as a second
        element."""
        V, N, T, cnt = self._extract_rows(iso, rng)
        sec = self.section(V[:cnt.nV], T[:cnt.nT], plane)
        return (sec, self.sample_property(sec.P)) if with_property else sec

    def section_profile(self, iso, normal, offsets, rng=None):
        """extract, then section_ladder(normal, offsets): the cross-section profile of the isosurface - (segments, length, area)."""
        V, N, T, cnt = self._extract_rows(iso, rng)
        return self.section_ladder(V[:cnt.nV], T[:cnt.nT], normal, offsets)

    # -- the grid resampled into a second device grid (mc33_hip.h: mc33hip_resample_grid) ------------------------------------------
    def _resampling(self, taps, stride, sigma):
        if sigma is not None:
            sig = (sigma,) * 3 if not hasattr(sigma, "__len__") else tuple(sigma)
            taps = tuple(gaussian_taps(x) for x in sig)
        r = Resampling()
        keep = []
        for a in range(3):
            if taps[a] is not None:
                w = (C.c_double * len(taps[a]))(*[float(x) for x in taps[a]])
                keep.append(w)
                r.taps[a] = C.cast(w, C.POINTER(C.c_double))
                r.ntaps[a] = len(taps[a])
            r.stride[a] = int(stride[a])
        return r, keep

    def resampled_size(self, taps=(None, None, None), stride=(1, 1, 1), sigma=None):
        """(npx', npy', npz') of what resampled() with these arguments returns; MC33Error(EINVAL) for what it refuses."""
        r, keep = self._resampling(taps, stride, sigma)
        n = (C.c_uint * 3)()
        _check(self.lib, self.lib.mc33hip_resampled_size(self.ctx, C.byref(r), C.byref(n)))
        return n[0], n[1], n[2]

    def resample_into(self, out, npx, taps=(None, None, None), stride=(1, 1, 1), sigma=None):
        """mc33hip_resample_grid into `out`, a device tensor [npz', npy', >= npx] of the grid's dtype used with its strides (any
        stride(1) >= npx, any stride(0)): only the grid points are written."""
        assert out.is_cuda and out.dim() == 3 and out.stride(2) == 1 and out.dtype == self.tensor.dtype and out.device == self.device
        r, keep = self._resampling(taps, stride, sigma)
        _check(self.lib, self.lib.mc33hip_resample_grid(self.ctx, C.byref(r), C.c_void_p(out.data_ptr()), out.stride(1), out.stride(0)))

    def resampled(self, taps=(None, None, None), stride=(1, 1, 1), sigma=None):
        """The grid resampled on the device - per axis a correlation with `taps` (an odd number of weights up to 17, None: none),
        edge samples replicated, then every stride-th point - into a new torch tensor [npz', npy', pitch'] with rows on 16-byte
        boundaries; `sigma` (a number or three, in samples) is shorthand for Gaussian taps (gaussian_taps).  Returns a new
        DeviceGrid over that tensor with the grid's r0, spacing d * stride, the current stream and the inclined matrices of this
        one.  Whole grids only (not a z-slab).  The definition is in include/mc33_hip.h."""
        import torch
        npx, npy, npz = self.resampled_size(taps, stride, sigma)
        sb = self.tensor.element_size()
        unit = max(1, 16 // sb)
        pitch = (npx + unit - 1) // unit * unit
        out = torch.empty((npz, npy, pitch), dtype=self.tensor.dtype, device=self.device)
        self.resample_into(out, npx, taps, stride, sigma)
        d = tuple(self.desc.d[k] * float(int(stride[k])) for k in range(3))
        g = DeviceGrid(out, r0=tuple(self.desc.r0), d=d, npx=npx)
        if getattr(self, "inclined", None):
            g.set_inclined(*self.inclined)
        return g

    # -- the grid rank-filtered into a second device grid (mc33_hip.h: mc33hip_rank_grid) ------------------------------------------
    @staticmethod
    def _ranking(rank, radius):
        rank = RANKS.get(rank, rank) if isinstance(rank, str) else int(rank)
        rad = (radius,) * 3 if not hasattr(radius, "__len__") else tuple(radius)
        if isinstance(rank, str) or len(rad) != 3 or any(int(x) < 0 for x in rad):
            raise ValueError("rank is 'min', 'median', 'max' or the integer; radius one number or three, none negative")
        return Ranking((C.c_uint * 3)(*[min(int(x), 0xFFFFFFFF) for x in rad]), rank)

    def rank_into(self, out, npx, rank="median", radius=(1, 1, 1)):
        """mc33hip_rank_grid into `out`, a device tensor [npz, npy, >= npx] of the grid's dtype used with its strides (any
        stride(1) >= npx, any stride(0)): only the grid points are written.  MC33Error(EINVAL) for what the library refuses."""
        assert out.is_cuda and out.dim() == 3 and out.stride(2) == 1 and out.dtype == self.tensor.dtype and out.device == self.device
        r = self._ranking(rank, radius)
        _check(self.lib, self.lib.mc33hip_rank_grid(self.ctx, C.byref(r), C.c_void_p(out.data_ptr()), out.stride(1), out.stride(0)))

    def ranked(self, rank="median", radius=(1, 1, 1)):
        """The grid rank-filtered on the device - every point replaced by the minimum, the median or the maximum of the box window
        of `radius` samples per axis x, y, z (one number: all three) around it, edge samples replicated; a selection, so the
        samples keep their bytes - into a new torch tensor [npz, npy, pitch] with rows on 16-byte boundaries.  `rank` is "min",
        "median", "max" or the integer; min and max take radii up to 8, the median up to 1 (3 x 3 x 3).  Returns a new DeviceGrid
        over that tensor with the grid's r0, d, the current stream and the inclined matrices of this one:
        grid.ranked("min", 1).ranked("max", 1) is an opening.  Whole grids only (not a z-slab).  The definition is in
        include/mc33_hip.h."""
        import torch
        npx, npy, npz = self.desc.npx, self.desc.npy, self.desc.npz_resident
        sb = self.tensor.element_size()
        unit = max(1, 16 // sb)
        pitch = (npx + unit - 1) // unit * unit
        out = torch.empty((npz, npy, pitch), dtype=self.tensor.dtype, device=self.device)
        self.rank_into(out, npx, rank, radius)
        g = DeviceGrid(out, r0=tuple(self.desc.r0), d=tuple(self.desc.d), npx=npx)
        if getattr(self, "inclined", None):
            g.set_inclined(*self.inclined)
        return g

    # -- the contour spectrum of the resident grid (mc33_hip.h: mc33hip_grid_spectrum) ----------------------------------------------
    def resident_range(self):
        """the cell slices whose planes are all resident: the whole grid, or a z-slab's own"""
        return Range(self.desc.plane0, self.desc.plane0 + self.desc.npz_resident - 1, 0, 0)

    def spectrum(self, isos, rng=None):
        """For up to 255 isovalues, strictly ascending as MC33_real: how many cells of cell slices rng (default: every slice
        whose planes are resident) the surface cuts at each, the histogram of the samples between them, the NaN samples and the
        range of the others - one pass over the grid, a few KB come back: a GridSpectrum.  MC33Error(EINVAL) for what the
        library refuses (include/mc33_hip.h)."""
        import numpy as np
        rng = rng or self.resident_range()
        isos = [float(x) for x in isos]
        n = len(isos)
        arr = (C.c_double * max(n, 1))(*isos)
        cut = np.zeros(n, np.uint64)
        hist = np.zeros(n + 1, np.uint64)
        a = Spectrum()
        a.isos, a.n = C.cast(arr, C.POINTER(C.c_double)), min(n, 0xFFFFFFFF)
        a.cut_cells = cut.ctypes.data_as(C.POINTER(C.c_ulonglong)) if n else None
        a.histogram = hist.ctypes.data_as(C.POINTER(C.c_ulonglong))
        _check(self.lib, self.lib.mc33hip_grid_spectrum(self.ctx, C.byref(rng), C.byref(a)))
        return GridSpectrum(isos, cut, hist, a.points, a.cells, a.nan_samples, a.sample_min, a.sample_max)

    def spectrum_ladder(self, n, rng=None):
        """The spectrum at n isovalues spread evenly strictly inside the range of the samples: a first call without isovalues
        finds that range, isovalue_ladder makes the steps.  ValueError when the samples have no range to spread steps over (a
        constant or all-NaN grid, infinite samples)."""
        first = self.spectrum([], rng)
        return self.spectrum(isovalue_ladder(first.sample_min, first.sample_max, n, self.dtype), rng)

    def probe_read(self, reps=10):
        """A plain read of the resident grid (nothing to do with an extraction): (best ms, median ms, bytes)."""
        best, med, nbytes = C.c_float(), C.c_float(), C.c_ulonglong()
        _check(self.lib, self.lib.mc33hip_probe_read(self.ctx, int(reps), C.byref(best), C.byref(med), C.byref(nbytes)))
        return best.value, med.value, nbytes.value

    def emit_shape(self):
        """The launch shape of the emit enqueued last (include/mc33_hip.h: mc33hip_emit_shape), for tests and tracing: an
        EmitShape; MC33Error(EINVAL) when the context has emitted nothing."""
        out = (C.c_ulonglong * 8)()
        _check(self.lib, self.lib.mc33hip_emit_shape(self.ctx, C.byref(out)))
        return EmitShape(*[int(x) for x in out])

    def tail_shape(self):
        """The shape of the tail of the last count or extraction (include/mc33_hip.h: mc33hip_tail_shape), for tests and
        tracing: a TailShape; MC33Error(EINVAL) when the context has counted nothing."""
        out = (C.c_ulonglong * 8)()
        _check(self.lib, self.lib.mc33hip_tail_shape(self.ctx, C.byref(out)))
        return TailShape(*[int(x) for x in out])

    def list_counts(self, n=1024):
        """The first n group cursors of the slow-cell list and of the dirty-segment list of that tail (mc33hip_list_counts):
        two uint32 arrays, valid until the next count."""
        import numpy as np
        slow, dirty = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        as_u = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))
        _check(self.lib, self.lib.mc33hip_list_counts(self.ctx, as_u(slow), as_u(dirty), n))
        return slow, dirty

    def timing(self):
        t = Timing()
        _check(self.lib, self.lib.mc33hip_last_timing(self.ctx, C.byref(t)))
        return t
