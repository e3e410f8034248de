"""ctypes binding of the C ABI in include/gpc_hip.h (libgpc_hip.so).

Plumbing only: numpy for host buffers, raw integer device pointers for HBM-resident
batches (typically torch tensors' data_ptr()).  There is no CPU fallback -- if the
shared library is missing or no gfx950 device is usable, this raises.
"""
import atexit
import ctypes as C
import os
import sys
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# GPC_HIP_LIB overrides the library path (used only to A/B differently compiled builds of this library)
LIB_PATH = os.environ.get("GPC_HIP_LIB") or os.path.join(HERE, "libgpc_hip.so")

MAX_TESTS = 32
MAX_GROUPS = 32   # GPC_MAX_GROUPS
OK, E_INVALID, E_NO_DEVICE, E_HIP, E_CAPACITY, E_NO_FOREST, E_FOREST_RANGE, E_IO, E_UNSUPPORTED = range(9)

SUPPORT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("d", "<f4")])
CORR_DTYPE = np.dtype([("src_x", "<i4"), ("src_y", "<i4"), ("tar_x", "<i4"), ("tar_y", "<i4")])
SCORE_MAX_THR = 8   # GPC_SCORE_MAX_THR
# gpc_score: exact counts per pair
SCORE_DTYPE = np.dtype([("n_records", "<i8"), ("n_ignored", "<i8"), ("n_no_truth", "<i8"), ("n_judged", "<i8"),
                        ("n_within", "<i8", (SCORE_MAX_THR,)), ("sum_e2_q8", "<i8"), ("n_candidates", "<i8"),
                        ("n_matchable", "<i8")])
# gpc_track: one row per track (gpc_hip_track_*)
TRACK_DTYPE = np.dtype([("first_pair", "<i4"), ("first_record", "<i4"), ("length", "<i4"), ("last_record", "<i4")])
# gpc_refinement: one per record (gpc_hip_refine_*); flags bit 0 evaluated, bit 1 minimum in x, bit 2 minimum in y
REFINEMENT_DTYPE = np.dtype([("dx_q8", "<i2"), ("dy_q8", "<i2"), ("cost", "<u2"), ("flags", "<u2")])
# gpc_quad: one closed circular match of a stereo sequence (gpc_hip_quads_*)
QUAD_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("d0", "<i4"), ("u", "<i4"), ("v", "<i4"), ("d1", "<i4"), ("support0", "<i4"),
                       ("support1", "<i4")])


class Settings(C.Structure):
    """gpc::inference::InferenceSettings (reference inference.hpp:71-131), same defaults."""
    _fields_ = [
        ("gradient_threshold", C.c_int32),
        ("disp_high", C.c_int32),
        ("vertical_tolerance", C.c_int32),
        ("epipolar_mode", C.c_int32),
        ("use_hashtable", C.c_int32),
        ("num_threads", C.c_int32),
    ]

    def __init__(self, gradient_threshold=10, disp_high=128, vertical_tolerance=1,
                 epipolar_mode=False, use_hashtable=False, num_threads=1):
        super().__init__(int(gradient_threshold), int(disp_high), int(vertical_tolerance),
                         int(bool(epipolar_mode)), int(bool(use_hashtable)), int(num_threads))

    @classmethod
    def sparsematch(cls):
        """The settings of samples/sparsematch.cpp:29-34."""
        return cls(5, 128, 0, True, False, 1)


class Truth(C.Structure):
    """gpc_truth: u / v / ignore planes, one [H][W] entry per pair (device pointers, or host pointers in the host forms)."""
    _fields_ = [("u", C.c_void_p), ("v", C.c_void_p), ("ignore", C.c_void_p)]


class FieldScorePrm(C.Structure):
    """gpc_field_score_prm: the parameters of the dense field scorer (gpc_hip_score_fields*); the documented defaults."""
    _fields_ = [("n_thr", C.c_int32), ("thr_q8", C.c_int32 * 8), ("out_abs_q8", C.c_int32), ("out_rel_pm", C.c_int32),
                ("n_speed", C.c_int32), ("speed_q8", C.c_int32 * 3), ("reserved", C.c_int32)]

    def __init__(self, thr_q8=(256, 768, 1280), out_abs_q8=768, out_rel_pm=50, speed_q8=(), n_thr=None, n_speed=None, reserved=0):
        thr_q8, speed_q8 = [int(t) for t in thr_q8], [int(t) for t in speed_q8]
        if len(thr_q8) > 8 or len(speed_q8) > 3:
            raise ValueError("at most 8 thresholds and 3 speed bounds")
        super().__init__(len(thr_q8) if n_thr is None else int(n_thr), (C.c_int32 * 8)(*thr_q8), int(out_abs_q8), int(out_rel_pm),
                         len(speed_q8) if n_speed is None else int(n_speed), (C.c_int32 * 3)(*speed_q8), int(reserved))


class FieldTally(C.Structure):
    """gpc_field_tally: exact counts and sums over judged pixels."""
    _fields_ = [("n_judged", C.c_int64), ("n_within", C.c_int64 * 8), ("n_outlier", C.c_int64), ("sum_e_q8", C.c_int64),
                ("sum_e2_q16", C.c_int64)]


class FieldScore(C.Structure):
    """gpc_field_score: one pair's counts.  The library returns counts only; the accessors divide them on the host, over all
    judged pixels or (bin = 0 .. 3) over one bin's, and return nan where nothing was judged."""
    _fields_ = [("n_pixels", C.c_int64), ("n_ignored", C.c_int64), ("n_no_truth", C.c_int64), ("n_hole", C.c_int64),
                ("all", FieldTally), ("bin", FieldTally * 4)]

    def tally(self, bin=None):
        return self.all if bin is None else self.bin[int(bin)]

    @staticmethod
    def _div(a, b):
        return float(a) / float(b) if b else float("nan")

    def epe(self, bin=None):
        """the mean end-point error in pixels"""
        t = self.tally(bin)
        return self._div(t.sum_e_q8, 256 * t.n_judged)

    def rms(self, bin=None):
        """the root of the mean squared error in pixels"""
        t = self.tally(bin)
        return self._div(t.sum_e2_q16, 65536 * t.n_judged) ** 0.5

    def within(self, k, bin=None):
        """the share of judged pixels within threshold k"""
        t = self.tally(bin)
        return self._div(t.n_within[int(k)], t.n_judged)

    def outlier_rate(self, bin=None):
        t = self.tally(bin)
        return self._div(t.n_outlier, t.n_judged)

    def density(self, bin=None):
        """judged pixels over the pixels that could be judged (judged + holes); a bin's share of them with bin given"""
        return self._div(self.tally(bin).n_judged, self.all.n_judged + self.n_hole)


class Consensus(C.Structure):
    """gpc_consensus: the parameters of the grid motion consensus filter (gpc_hip_consensus_*); the documented defaults."""
    _fields_ = [("cell", C.c_int32), ("shifts", C.c_int32), ("alpha_num", C.c_int32), ("alpha_den", C.c_int32)]

    def __init__(self, cell=16, shifts=4, alpha_num=6, alpha_den=1):
        super().__init__(int(cell), int(shifts), int(alpha_num), int(alpha_den))


DENSE_NONE = -2 ** 31   # GPC_DENSE_NONE: no block around the pixel holds min_count matches (its level is 255)


class Densify(C.Structure):
    """gpc_densify: the parameters of the hierarchical fill (gpc_hip_densify_*); the documented defaults."""
    _fields_ = [("max_level", C.c_int32), ("min_count", C.c_int32), ("spread", C.c_int32), ("max_cost", C.c_int32)]

    def __init__(self, max_level=15, min_count=1, spread=1, max_cost=0xFFFF):
        super().__init__(int(max_level), int(min_count), int(spread), int(max_cost))


class Clean(C.Structure):
    """gpc_clean: the parameters of the field cleaner (gpc_hip_clean_*); the documented defaults."""
    _fields_ = [("check_tol_q8", C.c_int32), ("speckle_diff_q8", C.c_int32), ("speckle_min", C.c_int32), ("median_radius", C.c_int32)]

    def __init__(self, check_tol_q8=256, speckle_diff_q8=256, speckle_min=64, median_radius=1):
        super().__init__(int(check_tol_q8), int(speckle_diff_q8), int(speckle_min), int(median_radius))


class Search(C.Structure):
    """gpc_search: the parameters of the local dense search (gpc_hip_search_*); the documented defaults."""
    _fields_ = [("radius", C.c_int32), ("range", C.c_int32), ("subpixel", C.c_int32), ("max_cost", C.c_int32)]

    def __init__(self, radius=2, range=1, subpixel=1, max_cost=0xFFFF):
        super().__init__(int(radius), int(range), int(subpixel), int(max_cost))


class Aggregate(C.Structure):
    """gpc_aggregate: the parameters of the scanline aggregation of the search's costs (gpc_hip_aggregate_*); the documented
    defaults.  The bits of paths: 1 left to right, 2 right to left, 4 top to bottom, 8 bottom to top."""
    _fields_ = [("radius", C.c_int32), ("range", C.c_int32), ("subpixel", C.c_int32), ("max_cost", C.c_int32), ("p1", C.c_int32),
                ("p2", C.c_int32), ("paths", C.c_int32)]

    def __init__(self, radius=2, range=1, subpixel=1, max_cost=0xFFFF, p1=128, p2=512, paths=15):
        super().__init__(int(radius), int(range), int(subpixel), int(max_cost), int(p1), int(p2), int(paths))


class Propagate(C.Structure):
    """gpc_propagate: the parameters of the propagation of field values between neighbours (gpc_hip_propagate_*); the
    documented defaults."""
    _fields_ = [("radius", C.c_int32), ("span", C.c_int32), ("iterations", C.c_int32), ("neighbours", C.c_int32)]

    def __init__(self, radius=2, span=1, iterations=6, neighbours=8):
        super().__init__(int(radius), int(span), int(iterations), int(neighbours))


class Gapfill(C.Structure):
    """gpc_gapfill: the parameters of the scanline hole closing (gpc_hip_gapfill_*); the documented defaults."""
    _fields_ = [("max_gap", C.c_int32), ("discon_q8", C.c_int32), ("select", C.c_int32), ("border", C.c_int32)]

    def __init__(self, max_gap=64, discon_q8=128, select=0, border=1):
        super().__init__(int(max_gap), int(discon_q8), int(select), int(border))


class Inpaint(C.Structure):
    """gpc_inpaint: the parameters of the guided completion (gpc_hip_inpaint_*); the documented defaults."""
    _fields_ = [("radius", C.c_int32), ("range_shift", C.c_int32), ("min_weight", C.c_int32), ("passes", C.c_int32)]

    def __init__(self, radius=4, range_shift=3, min_weight=512, passes=32):
        super().__init__(int(radius), int(range_shift), int(min_weight), int(passes))


class FilterMask(C.Structure):
    """gpc::inference::Forest::FilterMask (reference inference.hpp:137-156)."""
    _fields_ = [
        ("mask", C.c_int32 * (2 * MAX_TESTS)),
        ("tau", C.c_int32 * MAX_TESTS),
        ("num_tests", C.c_int32),
        ("type", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("discarded", C.c_int32),
    ]


class GpcError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("gpc_hip status %d: %s" % (status, msg))
        self.status = status


_lib = None

# every symbol include/gpc_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "gpc_hip_abi_version", "gpc_hip_status_string", "gpc_hip_device_count", "gpc_hip_create",
    "gpc_hip_destroy", "gpc_hip_last_error", "gpc_hip_set_stream", "gpc_hip_synchronize",
    "gpc_hip_reserve", "gpc_hip_set_arithmetic", "gpc_hip_host_alloc", "gpc_hip_host_free", "gpc_hip_read_forest", "gpc_hip_parse_forest", "gpc_hip_set_forest",
    "gpc_hip_read_forest_groups", "gpc_hip_parse_forest_groups", "gpc_hip_set_forest_groups", "gpc_hip_hash_codes_groups",
    "gpc_hip_warmup", "gpc_hip_preprocess", "gpc_hip_preprocess_begin", "gpc_hip_preprocess_fetch", "gpc_hip_resident_hits",
    "gpc_hip_rectified_match_begin", "gpc_hip_stereo_match_begin", "gpc_hip_match_pair_begin", "gpc_hip_match_fetch",
    "gpc_hip_hash_codes", "gpc_hip_rectified_match", "gpc_hip_stereo_match",
    "gpc_hip_match_pair", "gpc_hip_match_batch_device", "gpc_hip_set_pipeline", "gpc_hip_pipeline_join", "gpc_hip_match_batch",
    "gpc_hip_match_batch_device_packed", "gpc_hip_match_batch_packed", "gpc_hip_expand_packed", "gpc_hip_host_threads", "gpc_hip_host_numa_node", "gpc_hip_batch_stages", "gpc_hip_hash_plan", "gpc_hip_host_worker_cpus", "gpc_hip_fed_calls",
    "gpc_hip_enable_kernel_timing", "gpc_hip_set_kernel_timing_mask", "gpc_hip_reset_kernel_timing", "gpc_hip_kernel_count", "gpc_hip_kernel_slots",
    "gpc_hip_kernel_name", "gpc_hip_kernel_launch_name", "gpc_hip_kernel_time",
    "gpc_hip_train_set_create", "gpc_hip_train_set_destroy", "gpc_hip_train_set_size", "gpc_hip_train_set_marks",
    "gpc_hip_train_eval_split", "gpc_hip_train_mark_split_samples", "gpc_hip_train_fern",
    "gpc_hip_train_begin_fern", "gpc_hip_train_eval_level", "gpc_hip_train_commit_level", "gpc_hip_train_forest",
    "gpc_hip_extract_triplets", "gpc_hip_extract_triplets_device", "gpc_hip_train_set_read",
    "gpc_hip_match_sequence_device", "gpc_hip_match_sequence",
    "gpc_hip_score_supports_device", "gpc_hip_score_correspondences_device", "gpc_hip_score_batch_device",
    "gpc_hip_score_sequence_device", "gpc_hip_score_batch", "gpc_hip_score_sequence",
    "gpc_hip_score_supports", "gpc_hip_score_correspondences",
    "gpc_hip_track_records_device", "gpc_hip_track_sequence_device", "gpc_hip_track_records", "gpc_hip_track_sequence",
    "gpc_hip_consensus_supports_device", "gpc_hip_consensus_correspondences_device", "gpc_hip_consensus_batch_device",
    "gpc_hip_consensus_sequence_device", "gpc_hip_consensus_supports", "gpc_hip_consensus_correspondences",
    "gpc_hip_track_stream_create", "gpc_hip_track_stream_destroy", "gpc_hip_track_stream_reset",
    "gpc_hip_track_stream_push_device", "gpc_hip_track_stream_push", "gpc_hip_track_stream_push_records_device",
    "gpc_hip_track_stream_state", "gpc_hip_track_stream_table", "gpc_hip_track_stream_read_tracks",
    "gpc_hip_refine_supports_device", "gpc_hip_refine_correspondences_device", "gpc_hip_refine_batch_device",
    "gpc_hip_refine_sequence_device", "gpc_hip_refine_supports", "gpc_hip_refine_correspondences",
    "gpc_hip_pyramid_levels", "gpc_hip_pyramid_down_device", "gpc_hip_pyramid_merge_supports_device",
    "gpc_hip_pyramid_merge_correspondences_device", "gpc_hip_pyramid_batch_device", "gpc_hip_pyramid_sequence_device",
    "gpc_hip_pyramid_batch", "gpc_hip_pyramid_sequence",
    "gpc_hip_densify_supports_device", "gpc_hip_densify_correspondences_device", "gpc_hip_densify_batch_device",
    "gpc_hip_densify_sequence_device", "gpc_hip_densify_supports", "gpc_hip_densify_correspondences",
    "gpc_hip_quads_records_device", "gpc_hip_match_stereo_sequence_device", "gpc_hip_quads_sequence_device",
    "gpc_hip_quads_records", "gpc_hip_quads_sequence",
    "gpc_hip_clean_fields_device", "gpc_hip_flip_supports_device", "gpc_hip_flip_correspondences_device",
    "gpc_hip_clean_batch_device", "gpc_hip_clean_sequence_device", "gpc_hip_clean_fields",
    "gpc_hip_inpaint_fields_device", "gpc_hip_inpaint_batch_device", "gpc_hip_inpaint_sequence_device", "gpc_hip_inpaint_fields",
    "gpc_hip_search_fields_device", "gpc_hip_search_batch_device", "gpc_hip_search_sequence_device", "gpc_hip_search_fields",
    "gpc_hip_score_fields_device", "gpc_hip_score_fields",
    "gpc_hip_aggregate_fields_device", "gpc_hip_aggregate_batch_device", "gpc_hip_aggregate_sequence_device",
    "gpc_hip_aggregate_fields",
    "gpc_hip_propagate_fields_device", "gpc_hip_propagate_fields",
    "gpc_hip_gapfill_fields_device", "gpc_hip_gapfill_fields",
]


def load():
    """Loads libgpc_hip.so (built by opengpc_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            "%s is missing: build it with `python -m opengpc_amd.build` (needs hipcc). "
            "There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.gpc_hip_status_string.restype = C.c_char_p
    L.gpc_hip_last_error.restype = C.c_char_p
    L.gpc_hip_last_error.argtypes = [C.c_void_p]
    L.gpc_hip_kernel_name.restype = C.c_char_p
    L.gpc_hip_kernel_launch_name.restype = C.c_char_p
    L.gpc_hip_kernel_launch_name.argtypes = [C.c_void_p, C.c_int]
    L.gpc_hip_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.gpc_hip_destroy.argtypes = [C.c_void_p]
    L.gpc_hip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.gpc_hip_synchronize.argtypes = [C.c_void_p]
    L.gpc_hip_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.gpc_hip_set_arithmetic.argtypes = [C.c_void_p, C.c_int]
    L.gpc_hip_host_alloc.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.gpc_hip_host_free.argtypes = [C.c_void_p, C.c_void_p]
    L.gpc_hip_read_forest.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(FilterMask)]
    L.gpc_hip_parse_forest.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(FilterMask)]
    L.gpc_hip_set_forest.argtypes = [C.c_void_p, C.POINTER(FilterMask)]
    L.gpc_hip_read_forest_groups.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(FilterMask), C.c_int, C.POINTER(C.c_int)]
    L.gpc_hip_parse_forest_groups.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(FilterMask), C.c_int, C.POINTER(C.c_int)]
    L.gpc_hip_set_forest_groups.argtypes = [C.c_void_p, C.POINTER(FilterMask), C.c_int]
    L.gpc_hip_hash_codes_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.gpc_hip_preprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.gpc_hip_warmup.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Settings)]
    L.gpc_hip_preprocess_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.gpc_hip_preprocess_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.gpc_hip_resident_hits.argtypes = [C.c_void_p]
    L.gpc_hip_hash_codes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    pre = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
           C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.gpc_hip_rectified_match.argtypes = pre
    L.gpc_hip_stereo_match.argtypes = pre
    L.gpc_hip_rectified_match_begin.argtypes = pre[:12]
    L.gpc_hip_stereo_match_begin.argtypes = pre[:12]
    L.gpc_hip_match_pair_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Settings)]
    L.gpc_hip_match_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int)]
    L.gpc_hip_match_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                     C.POINTER(Settings), C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                     C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.gpc_hip_match_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(Settings), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.gpc_hip_match_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(Settings), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.gpc_hip_match_sequence_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings),
                                                C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.gpc_hip_match_sequence.argtypes = L.gpc_hip_match_sequence_device.argtypes
    rec = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Truth), C.c_void_p, C.c_int,
           C.c_void_p]
    L.gpc_hip_score_supports_device.argtypes = rec
    L.gpc_hip_score_correspondences_device.argtypes = rec
    L.gpc_hip_score_supports.argtypes = rec
    L.gpc_hip_score_correspondences.argtypes = rec
    L.gpc_hip_score_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings),
                                             C.POINTER(Truth), C.c_void_p, C.c_int, C.c_void_p]
    L.gpc_hip_score_batch.argtypes = L.gpc_hip_score_batch_device.argtypes
    L.gpc_hip_score_sequence_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings),
                                                C.POINTER(Truth), C.c_void_p, C.c_int, C.c_void_p]
    L.gpc_hip_score_sequence.argtypes = L.gpc_hip_score_sequence_device.argtypes
    L.gpc_hip_track_records_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.gpc_hip_track_records.argtypes = L.gpc_hip_track_records_device.argtypes
    L.gpc_hip_track_sequence_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_void_p,
                                                C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_void_p]
    L.gpc_hip_track_sequence.argtypes = L.gpc_hip_track_sequence_device.argtypes
    L.gpc_hip_track_stream_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Settings), C.c_int, C.c_int,
                                              C.POINTER(C.c_void_p)]
    L.gpc_hip_track_stream_destroy.argtypes = [C.c_void_p, C.c_void_p]
    L.gpc_hip_track_stream_reset.argtypes = [C.c_void_p, C.c_void_p]
    L.gpc_hip_track_stream_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.gpc_hip_track_stream_push.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int32)]
    L.gpc_hip_track_stream_push_records_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                           C.c_void_p]
    L.gpc_hip_track_stream_state.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int32)]
    L.gpc_hip_track_stream_table.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.gpc_hip_track_stream_read_tracks.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]
    L.gpc_hip_consensus_supports_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                    C.POINTER(Consensus), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.gpc_hip_consensus_correspondences_device.argtypes = L.gpc_hip_consensus_supports_device.argtypes
    L.gpc_hip_consensus_supports.argtypes = L.gpc_hip_consensus_supports_device.argtypes
    L.gpc_hip_consensus_correspondences.argtypes = L.gpc_hip_consensus_supports_device.argtypes
    L.gpc_hip_consensus_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings),
                                                 C.POINTER(Consensus), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_consensus_sequence_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings),
                                                    C.POINTER(Consensus), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_refine_supports_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                 C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.gpc_hip_refine_supports.argtypes = L.gpc_hip_refine_supports_device.argtypes
    L.gpc_hip_refine_correspondences_device.argtypes = L.gpc_hip_refine_supports_device.argtypes[:11]
    L.gpc_hip_refine_correspondences.argtypes = L.gpc_hip_refine_correspondences_device.argtypes
    L.gpc_hip_refine_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings),
                                              C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_refine_sequence_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_int,
                                                 C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_pyramid_levels.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.gpc_hip_pyramid_down_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.gpc_hip_pyramid_merge_supports_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                        C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.gpc_hip_pyramid_merge_correspondences_device.argtypes = L.gpc_hip_pyramid_merge_supports_device.argtypes
    L.gpc_hip_pyramid_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.POINTER(Settings), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_pyramid_batch.argtypes = L.gpc_hip_pyramid_batch_device.argtypes
    L.gpc_hip_pyramid_sequence_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Settings),
                                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_pyramid_sequence.argtypes = L.gpc_hip_pyramid_sequence_device.argtypes
    L.gpc_hip_densify_supports_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(Densify), C.c_void_p, C.c_void_p]
    L.gpc_hip_densify_correspondences_device.argtypes = L.gpc_hip_densify_supports_device.argtypes
    L.gpc_hip_densify_supports.argtypes = L.gpc_hip_densify_supports_device.argtypes
    L.gpc_hip_densify_correspondences.argtypes = L.gpc_hip_densify_supports_device.argtypes
    L.gpc_hip_densify_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings),
                                               C.c_int, C.POINTER(Densify), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_densify_sequence_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_int,
                                                  C.POINTER(Densify), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_match_batch_device_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                    C.POINTER(Settings), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]
    L.gpc_hip_match_batch_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_expand_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.gpc_hip_host_threads.argtypes = [C.c_void_p]
    L.gpc_hip_host_numa_node.argtypes = [C.c_void_p]
    L.gpc_hip_fed_calls.argtypes = [C.c_void_p]
    L.gpc_hip_set_pipeline.argtypes = [C.c_void_p, C.c_int]
    L.gpc_hip_pipeline_join.argtypes = [C.c_void_p]
    L.gpc_hip_batch_stages.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.gpc_hip_hash_plan.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.gpc_hip_host_worker_cpus.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    L.gpc_hip_enable_kernel_timing.argtypes = [C.c_void_p, C.c_int]
    L.gpc_hip_set_kernel_timing_mask.argtypes = [C.c_void_p, C.c_uint]
    L.gpc_hip_reset_kernel_timing.argtypes = [C.c_void_p]
    L.gpc_hip_kernel_time.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    vp, ci = C.c_void_p, C.c_int
    L.gpc_hip_train_set_create.argtypes = [vp, vp, ci, C.POINTER(C.c_void_p)]
    L.gpc_hip_train_set_destroy.argtypes = [vp, vp]
    L.gpc_hip_train_set_size.argtypes = [vp]
    L.gpc_hip_train_set_marks.argtypes = [vp, vp, vp, vp]
    L.gpc_hip_train_eval_split.argtypes = [vp, vp, vp, ci, C.c_double, vp]
    L.gpc_hip_train_mark_split_samples.argtypes = [vp, vp, vp, ci]
    L.gpc_hip_train_fern.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, C.c_double, vp, vp]
    L.gpc_hip_train_begin_fern.argtypes = [vp, vp, ci]
    L.gpc_hip_train_eval_level.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp]
    L.gpc_hip_train_commit_level.argtypes = [vp, vp, vp, ci]
    L.gpc_hip_train_forest.argtypes = [vp, vp, ci, ci, vp, ci, ci, ci, ci, C.c_double, vp, ci, vp, vp]
    L.gpc_hip_extract_triplets.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.gpc_hip_extract_triplets_device.argtypes = L.gpc_hip_extract_triplets.argtypes
    L.gpc_hip_train_set_read.argtypes = [vp, vp, ci, ci, vp]
    L.gpc_hip_quads_records_device.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp, vp, ci, ci, ci, ci, vp, ci, vp]
    L.gpc_hip_quads_records.argtypes = L.gpc_hip_quads_records_device.argtypes
    L.gpc_hip_match_stereo_sequence_device.argtypes = [vp, vp, vp, ci, ci, ci, C.POINTER(Settings), C.POINTER(Settings), vp, ci, vp, vp,
                                                       vp, ci, vp, vp, vp]
    L.gpc_hip_quads_sequence_device.argtypes = [vp, vp, vp, ci, ci, ci, C.POINTER(Settings), C.POINTER(Settings), ci, vp, ci, vp, vp,
                                                vp, ci, vp, vp, vp, vp, ci, vp]
    L.gpc_hip_quads_sequence.argtypes = L.gpc_hip_quads_sequence_device.argtypes
    L.gpc_hip_debug_live_resources.argtypes = [C.POINTER(C.c_uint64)]
    L.gpc_hip_clean_fields_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Clean),
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_clean_fields.argtypes = L.gpc_hip_clean_fields_device.argtypes
    L.gpc_hip_flip_supports_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.gpc_hip_flip_correspondences_device.argtypes = L.gpc_hip_flip_supports_device.argtypes
    L.gpc_hip_clean_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_int,
                                             C.POINTER(Densify), C.POINTER(Clean)] + [C.c_void_p] * 8
    L.gpc_hip_clean_sequence_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_int,
                                                C.POINTER(Densify), C.POINTER(Clean)] + [C.c_void_p] * 8
    L.gpc_hip_inpaint_fields_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Inpaint),
                                                C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_inpaint_fields.argtypes = L.gpc_hip_inpaint_fields_device.argtypes
    L.gpc_hip_inpaint_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_int,
                                               C.POINTER(Densify), C.POINTER(Clean), C.POINTER(Inpaint)] + [C.c_void_p] * 11
    L.gpc_hip_inpaint_sequence_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_int,
                                                  C.POINTER(Densify), C.POINTER(Clean), C.POINTER(Inpaint)] + [C.c_void_p] * 11
    L.gpc_hip_search_fields_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.POINTER(Search), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_search_fields.argtypes = L.gpc_hip_search_fields_device.argtypes
    L.gpc_hip_search_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_int,
                                              C.POINTER(Densify), C.POINTER(Search), C.POINTER(Clean)] + [C.c_void_p] * 9
    L.gpc_hip_search_sequence_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_int,
                                                 C.POINTER(Densify), C.POINTER(Search), C.POINTER(Clean)] + [C.c_void_p] * 9
    L.gpc_hip_aggregate_fields_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(Aggregate), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_aggregate_fields.argtypes = L.gpc_hip_aggregate_fields_device.argtypes
    L.gpc_hip_propagate_fields_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(Propagate), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_propagate_fields.argtypes = L.gpc_hip_propagate_fields_device.argtypes
    L.gpc_hip_gapfill_fields_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Gapfill),
                                                C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_gapfill_fields.argtypes = L.gpc_hip_gapfill_fields_device.argtypes
    L.gpc_hip_aggregate_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_int,
                                                 C.POINTER(Densify), C.POINTER(Aggregate), C.POINTER(Clean)] + [C.c_void_p] * 9
    L.gpc_hip_aggregate_sequence_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Settings), C.c_int,
                                                    C.POINTER(Densify), C.POINTER(Aggregate), C.POINTER(Clean)] + [C.c_void_p] * 9
    L.gpc_hip_score_fields_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Truth),
                                              C.POINTER(FieldScorePrm), C.c_void_p, C.c_void_p, C.c_void_p]
    L.gpc_hip_score_fields.argtypes = L.gpc_hip_score_fields_device.argtypes
    _lib = L
    return L


def _check(L, ctx, status, allow=()):
    if status == OK or status in allow:
        return status
    msg = L.gpc_hip_status_string(status).decode()
    if status == E_HIP and ctx:
        msg += ": " + L.gpc_hip_last_error(ctx).decode()
    raise GpcError(status, msg)


def live_resources():
    """(device blocks, device bytes, page-locked blocks, streams + events) the library holds right now, over every context
    of the process (gpc_hip_debug_live_resources); what callers own through pinned_empty is not counted"""
    out = (C.c_uint64 * 4)()
    _check(load(), None, load().gpc_hip_debug_live_resources(out))
    return tuple(int(v) for v in out)


def expand_packed(packed, rows, n):
    """Host-side expansion of one pair's packed supports (gpc_hip_expand_packed) -> SUPPORT_DTYPE array of n records."""
    L = load()
    packed = np.ascontiguousarray(packed, np.uint32)
    rows = np.ascontiguousarray(rows, np.int32)
    out = np.empty(max(int(n), 1), SUPPORT_DTYPE)
    st = L.gpc_hip_expand_packed(_ptr(packed), _ptr(rows), len(rows), int(n), _ptr(out))
    _check(L, None, st)
    return out[:int(n)]


def read_forest(path, width, height):
    """Forest::readForest.  Returns (status, FilterMask); a missing file gives (E_IO, empty mask)."""
    L = load()
    fm = FilterMask()
    st = L.gpc_hip_read_forest(os.fsencode(path), width, height, C.byref(fm))
    return st, fm


def parse_forest(text, width, height):
    L = load()
    fm = FilterMask()
    st = L.gpc_hip_parse_forest(text.encode(), width, height, C.byref(fm))
    return st, fm


def _forest_groups(fn, arg, width, height):
    L = load()
    arr = (FilterMask * MAX_GROUPS)()
    n = C.c_int(0)
    st = fn(arg, width, height, arr, MAX_GROUPS, C.byref(n))
    return st, [arr[i] for i in range(min(n.value, MAX_GROUPS))] if st == OK else []


def read_forest_groups(path, width, height):
    """The forest's ferns packed into groups of <= 32 tests (gpc_hip_read_forest_groups).  Returns (status, [FilterMask])."""
    return _forest_groups(load().gpc_hip_read_forest_groups, os.fsencode(path), width, height)


def parse_forest_groups(text, width, height):
    return _forest_groups(load().gpc_hip_parse_forest_groups, text.encode(), width, height)


# training (include/gpc_hip.h): gpc_split = the scoring fields of Feature::params; gpc_split_stats = splitStats
SPLIT_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("tau", "<i4")])
STATS_DTYPE = np.dtype([("prec", "<f8"), ("rec", "<f8"), ("hmean", "<f8"), ("convcomb", "<f8"),
                        ("tp", "<i4"), ("fp", "<i4"), ("fn", "<i4"), ("tot", "<i4")])
PATCH_BYTES = 729
# gpc_triplet_points: the reference point in the left frame, the positive and the negative point in the right frame
POINTS_DTYPE = np.dtype([("rx", "<i4"), ("ry", "<i4"), ("px", "<i4"), ("py", "<i4"), ("nx", "<i4"), ("ny", "<i4")])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def pyramid_levels(width, height, levels):
    """(status, widths, heights) of gpc_hip_pyramid_levels: the sizes of the levels of a width x height image, host only"""
    n = max(int(levels), 1)
    ws, hs = np.zeros(n, np.int32), np.zeros(n, np.int32)
    st = load().gpc_hip_pyramid_levels(int(width), int(height), int(levels), _ptr(ws), _ptr(hs))
    return st, ws, hs


def kept_count(pts, width, height):
    """triplets that gpc_hip_extract_triplets keeps: all three points x > 20 && y > 20 && x < width-20 && y < height-20
    (Feature.hpp:208-214)"""
    p = np.asarray(pts, POINTS_DTYPE)
    ok = np.ones(len(p), bool)
    for x, y in (("rx", "ry"), ("px", "py"), ("nx", "ny")):
        ok &= (p[x] > 20) & (p[y] > 20) & (p[x] < width - 20) & (p[y] < height - 20)
    return int(ok.sum())


def _device_frames(a, b, device):
    """True for torch.uint8 tensors on GPU `device` (the _device entry point reads them where they lie); False for host
    frames.  Tensors on another GPU, of another dtype or not contiguous are refused: the kernels would read them as raw
    bytes, or fault on an address the GPU cannot reach."""
    ta, tb = hasattr(a, "data_ptr") and hasattr(a, "is_cuda"), hasattr(b, "data_ptr") and hasattr(b, "is_cuda")
    if not (ta or tb):
        return False
    if not (ta and tb):
        raise ValueError("rawL / rawR: both tensors or both arrays")
    import torch
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise ValueError("rawL / rawR: torch.uint8 tensors (got %s, %s)" % (a.dtype, b.dtype))
    if a.is_cuda != b.is_cuda:
        raise ValueError("rawL / rawR: both on the GPU or both on the host")
    if not a.is_cuda:
        return False
    if a.device.index != device or b.device.index != device:
        raise ValueError("rawL / rawR: tensors on cuda:%d, the context's device (got %s, %s)" % (device, a.device, b.device))
    if not (a.is_contiguous() and b.is_contiguous()):
        raise ValueError("rawL / rawR: contiguous tensors")
    return True


def _host_frames(a):
    """uint8 host frames as a C-contiguous numpy array (CPU tensors included); other dtypes are refused, not converted"""
    if hasattr(a, "data_ptr") and hasattr(a, "numpy"):
        a = a.detach().numpy()
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise ValueError("rawL / rawR: uint8 frames (got %s)" % a.dtype)
    return np.ascontiguousarray(a)


def score_thresholds(thr):
    """thresholds as the float32 array the library takes: 1 .. 8 values, each finite and >= 0 (ValueError otherwise)"""
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(thr, np.float32)))
    if t.ndim != 1 or not 1 <= len(t) <= SCORE_MAX_THR:
        raise ValueError("thresholds: between 1 and %d values" % SCORE_MAX_THR)
    if not np.isfinite(t).all() or (t < 0).any():
        raise ValueError("thresholds: finite and >= 0")
    return t


def _host_truth(u, v, ignore, shape, flow):
    """host truth planes of `shape` = (P, H, W) as contiguous arrays (float32 u, v; uint8 ignore); supports take no v"""
    if flow and v is None:
        raise ValueError("truth: correspondences need v")
    if not flow and v is not None:
        raise ValueError("truth: v must be None for supports")
    out = []
    for name, a, dt in (("u", u, np.float32), ("v", v, np.float32), ("ignore", ignore, np.uint8)):
        if a is None:
            if name == "u":
                raise ValueError("truth: u is needed")
            out.append(None)
            continue
        a = np.asarray(a)
        if a.dtype != dt:
            raise ValueError("truth %s: %s planes (got %s)" % (name, np.dtype(dt).name, a.dtype))
        if a.shape != tuple(shape):
            raise ValueError("truth %s: shape %s, expected %s" % (name, a.shape, tuple(shape)))
        out.append(np.ascontiguousarray(a))
    return out


_live_contexts = weakref.WeakSet()


def _close_live_contexts():
    """Contexts still open at interpreter exit are closed here, while the HIP runtime is still up;
    a destructor that reaches the library during interpreter teardown could otherwise call into a
    runtime that is already being destroyed."""
    for c in list(_live_contexts):
        try:
            c.close()
        except Exception:
            pass


atexit.register(_close_live_contexts)


class Context:
    """One gpc_hip_ctx: one device, one stream, one host thread at a time."""

    def __init__(self, device=0):
        self.L = load()
        self.h = None
        h = C.c_void_p()
        _check(self.L, None, self.L.gpc_hip_create(device, C.byref(h)))
        self.h = h
        self.device = device
        self._pinned = []
        _live_contexts.add(self)

    def close(self):
        if self.h:
            for p in self._pinned:
                self.L.gpc_hip_host_free(self.h, p)
            self._pinned = []
            self.L.gpc_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():  # atexit already closed what was open; never call HIP from teardown
            return
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st, allow=()):
        return _check(self.L, self.h, st, allow)

    # ---- setup
    def set_stream(self, stream_ptr):
        self._ck(self.L.gpc_hip_set_stream(self.h, C.c_void_p(stream_ptr or 0)))

    def synchronize(self):
        self._ck(self.L.gpc_hip_synchronize(self.h))

    def reserve(self, width, height, max_pairs):
        self._ck(self.L.gpc_hip_reserve(self.h, width, height, max_pairs))

    def pinned_empty(self, shape, dtype):
        """numpy array in page-locked host memory (gpc_hip_host_alloc); freed with the context."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        self._ck(self.L.gpc_hip_host_alloc(self.h, max(nbytes, 1), C.byref(p)))
        self._pinned.append(p)
        buf = (C.c_uint8 * max(nbytes, 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def set_arithmetic(self, naive):
        """False: the reference's default SSE build; True: its SSE=OFF (*Naive) arithmetic."""
        self._ck(self.L.gpc_hip_set_arithmetic(self.h, 1 if naive else 0))

    def set_forest(self, fm):
        self._ck(self.L.gpc_hip_set_forest(self.h, C.byref(fm)))
        self._ngroups = 1

    def set_forest_groups(self, groups):
        """Group mode (gpc_hip_set_forest_groups): every group matches as a forest of its own, the results are their union."""
        arr = (FilterMask * len(groups))(*groups)
        self._ck(self.L.gpc_hip_set_forest_groups(self.h, arr, len(groups)))
        self._ngroups = len(groups)

    def load_forest_groups(self, path, width, height):
        st, groups = read_forest_groups(path, width, height)
        _check(self.L, None, st)
        self.set_forest_groups(groups)
        return groups

    def hash_codes_groups(self, smooth, grad):
        """Dense code images of every group of the current forest: (n_groups, H, W) uint32."""
        smooth = np.ascontiguousarray(smooth, np.uint8)
        grad = np.ascontiguousarray(grad, np.uint8)
        H, W = smooth.shape
        codes = np.empty((getattr(self, "_ngroups", 1), H, W), np.uint32)
        self._ck(self.L.gpc_hip_hash_codes_groups(self.h, _ptr(smooth), _ptr(grad), W, H, _ptr(codes)))
        return codes

    def load_forest(self, path, width, height):
        st, fm = read_forest(path, width, height)
        _check(self.L, None, st)
        self.set_forest(fm)
        return fm

    # ---- host-buffer entry points
    def preprocess(self, raw, threshold):
        raw = np.ascontiguousarray(raw, np.uint8)
        H, W = raw.shape
        smooth = np.empty((H, W), np.uint8)
        grad = np.empty((H, W), np.uint8)
        mask = np.empty(W * H, np.int32)
        n = C.c_int()
        self._ck(self.L.gpc_hip_preprocess(self.h, _ptr(raw), W, H, int(threshold), _ptr(smooth), _ptr(grad),
                                           _ptr(mask), mask.size, C.byref(n)))
        return smooth, grad, mask[:n.value].copy()

    def preprocess_resident(self, raw, threshold):
        """gpc_hip_preprocess_begin + _fetch: the arrays returned are the ones the library filled and remembers as the
        host copies of the image it keeps on the device -- hand THEM (not copies) to rectified_match / stereo_match and
        the match runs from the resident image (resident_hits() counts those calls)."""
        raw = np.ascontiguousarray(raw, np.uint8)
        H, W = raw.shape
        self._ck(self.L.gpc_hip_preprocess_begin(self.h, _ptr(raw), W, H, int(threshold)))
        smooth = np.empty((H, W), np.uint8)
        grad = np.empty((H, W), np.uint8)
        full = np.empty((W - 26) * (H - 26), np.int32)    # (allocated while the device works)
        n = C.c_int()
        self._ck(self.L.gpc_hip_preprocess_fetch(self.h, _ptr(smooth), _ptr(grad), _ptr(full), full.size, C.byref(n)))
        return smooth, grad, full[:n.value]      # a view: the same address the library remembers

    def match_async(self, kind, a, b, settings, cap=None):
        """The two-step forms: kind 'rectified' / 'stereo' on (smooth, grad, mask) triples, 'pair' on raw images.
        Returns (records, true count, status, (candidates L, candidates R) or None)."""
        s_ = settings
        if kind == "pair":
            a = np.ascontiguousarray(a, np.uint8)
            b = np.ascontiguousarray(b, np.uint8)
            H, W = a.shape
            self._ck(self.L.gpc_hip_match_pair_begin(self.h, _ptr(a), _ptr(b), W, H, C.byref(s_)))
            dtype = SUPPORT_DTYPE
        else:
            (sl, gl, ml), (sr, gr, mr) = a, b
            H, W = sl.shape
            fn = self.L.gpc_hip_rectified_match_begin if kind == "rectified" else self.L.gpc_hip_stereo_match_begin
            self._ck(fn(self.h, _ptr(sl), _ptr(gl), _ptr(ml), len(ml), _ptr(sr), _ptr(gr), _ptr(mr), len(mr), W, H, C.byref(s_)))
            dtype = SUPPORT_DTYPE if kind == "rectified" else CORR_DTYPE
        cap = cap if cap is not None else W * H * getattr(self, "_ngroups", 1)
        out = np.empty(max(cap, 1), dtype)
        n, nl, nr = C.c_int(), C.c_int(-1), C.c_int(-1)
        st = self._ck(self.L.gpc_hip_match_fetch(self.h, _ptr(out), cap, C.byref(n), C.byref(nl), C.byref(nr)), allow=(E_CAPACITY,))
        if st == E_CAPACITY:     # the results stay until the next call: fetch again with room for all of them
            big = np.empty(n.value, dtype)
            self._ck(self.L.gpc_hip_match_fetch(self.h, _ptr(big), n.value, C.byref(n), C.byref(nl), C.byref(nr)))
            assert np.array_equal(big[:cap].view(np.uint8), out[:cap].view(np.uint8))
        return out[:min(n.value, cap)].copy(), n.value, st, ((nl.value, nr.value) if kind == "pair" else None)

    def batch_stages(self):
        """ms since entry of the last match_batch / match_batch_packed call: upload seen done, kernels done, last packed
        chunk landed, delivery done (gpc_hip_batch_stages)."""
        a = (C.c_float * 4)()
        self.L.gpc_hip_batch_stages(self.h, a)
        return [float(v) for v in a]

    def hash_plan(self):
        """(tile rows, tiles per workgroup, workgroups per tile column, first workgroup of the last round) of the context's
        most recent k_hash launch (gpc_hip_hash_plan); raises GpcError (E_INVALID) before the first one."""
        a = (C.c_int32 * 4)()
        self._ck(self.L.gpc_hip_hash_plan(self.h, a))
        return tuple(int(v) for v in a)

    def worker_cpus(self):
        a = (C.c_int * 64)()
        n = self.L.gpc_hip_host_worker_cpus(self.h, a, 64)
        return [int(a[i]) for i in range(min(n, 64))]

    def resident_hits(self):
        return self.L.gpc_hip_resident_hits(self.h)

    def warmup(self, width, height, settings=None):
        """gpc_hip_warmup: first-use costs of a pair of this size, paid now (the forest must be set)."""
        self._ck(self.L.gpc_hip_warmup(self.h, width, height, C.byref(settings) if settings is not None else None))

    def hash_codes(self, smooth, grad):
        smooth = np.ascontiguousarray(smooth, np.uint8)
        grad = np.ascontiguousarray(grad, np.uint8)
        H, W = smooth.shape
        codes = np.empty((H, W), np.uint32)
        self._ck(self.L.gpc_hip_hash_codes(self.h, _ptr(smooth), _ptr(grad), W, H, _ptr(codes)))
        return codes

    def _match_pre(self, fn, dtype, L_img, R_img, settings, cap):
        (sl, gl, ml), (sr, gr, mr) = L_img, R_img
        sl, gl, sr, gr = [np.ascontiguousarray(a, np.uint8) for a in (sl, gl, sr, gr)]
        ml = np.ascontiguousarray(ml, np.int32)
        mr = np.ascontiguousarray(mr, np.int32)
        H, W = sl.shape
        cap = cap if cap is not None else W * H * getattr(self, "_ngroups", 1)
        out = np.empty(max(cap, 1), dtype)
        n = C.c_int()
        st = fn(self.h, _ptr(sl), _ptr(gl), _ptr(ml), len(ml), _ptr(sr), _ptr(gr), _ptr(mr), len(mr), W, H,
                C.byref(settings), _ptr(out), cap, C.byref(n))
        self._ck(st, allow=(E_CAPACITY,))
        return out[:min(n.value, cap)].copy(), n.value, st

    def rectified_match(self, L_img, R_img, settings, cap=None):
        """Forest::rectifiedMatch on (smooth, grad, mask) triples."""
        return self._match_pre(self.L.gpc_hip_rectified_match, SUPPORT_DTYPE, L_img, R_img, settings, cap)

    def stereo_match(self, L_img, R_img, settings, cap=None):
        """Forest::stereoMatch on (smooth, grad, mask) triples."""
        return self._match_pre(self.L.gpc_hip_stereo_match, CORR_DTYPE, L_img, R_img, settings, cap)

    def match_pair(self, rawL, rawR, settings, cap=None):
        rawL = np.ascontiguousarray(rawL, np.uint8)
        rawR = np.ascontiguousarray(rawR, np.uint8)
        H, W = rawL.shape
        cap = cap if cap is not None else W * H * getattr(self, "_ngroups", 1)
        out = np.empty(max(cap, 1), SUPPORT_DTYPE)
        n, nl, nr = C.c_int(), C.c_int(), C.c_int()
        st = self.L.gpc_hip_match_pair(self.h, _ptr(rawL), _ptr(rawR), W, H, C.byref(settings), _ptr(out), cap,
                                       C.byref(n), C.byref(nl), C.byref(nr))
        self._ck(st, allow=(E_CAPACITY,))
        return out[:min(n.value, cap)].copy(), n.value, (nl.value, nr.value), st

    def match_batch(self, rawL, rawR, settings, cap, out=None):
        rawL = np.ascontiguousarray(rawL, np.uint8)
        rawR = np.ascontiguousarray(rawR, np.uint8)
        P, H, W = rawL.shape
        if out is None:
            out = np.empty((P, cap), SUPPORT_DTYPE)
        counts = np.empty(P, np.int32)
        ncand = np.empty((P, 2), np.int32)
        st = self.L.gpc_hip_match_batch(self.h, _ptr(rawL), _ptr(rawR), W, H, P, C.byref(settings), _ptr(out), cap,
                                        _ptr(counts), _ptr(ncand))
        self._ck(st, allow=(E_CAPACITY,))
        return out, counts, ncand, st

    def match_batch_packed(self, rawL, rawR, settings, cap, packed=None, rows=None):
        """Host images -> PACKED results in host memory (gpc_hip_match_batch_packed): words xL | xR << 16 [P][cap], per-row
        counts [P][H], true counts [P], candidate counts [P][2]; expand_packed() makes a pair's ndb::Support records."""
        rawL = np.ascontiguousarray(rawL, np.uint8)
        rawR = np.ascontiguousarray(rawR, np.uint8)
        P, H, W = rawL.shape
        if packed is None:
            packed = np.empty((P, cap), np.uint32)
        if rows is None:
            rows = np.empty((P, H), np.int32)
        counts = np.empty(P, np.int32)
        ncand = np.empty((P, 2), np.int32)
        st = self.L.gpc_hip_match_batch_packed(self.h, _ptr(rawL), _ptr(rawR), W, H, P, C.byref(settings), _ptr(packed), cap,
                                               _ptr(rows), _ptr(counts), _ptr(ncand))
        self._ck(st, allow=(E_CAPACITY,))
        return packed, rows, counts, ncand, st

    # ---- device-resident batch (pointers are integers, e.g. torch.Tensor.data_ptr())
    def match_batch_device(self, d_rawL, d_rawR, width, height, npairs, settings, d_out, cap_per_pair,
                           d_counts, d_ncand=0):
        self._ck(self.L.gpc_hip_match_batch_device(self.h, C.c_void_p(d_rawL), C.c_void_p(d_rawR), width, height,
                                                   npairs, C.byref(settings), C.c_void_p(d_out), cap_per_pair,
                                                   C.c_void_p(d_counts), C.c_void_p(d_ncand or 0)))

    def set_pipeline(self, lanes):
        """2: consecutive match_batch_device calls alternate between two lanes (gpc_hip_set_pipeline); 1: strict."""
        self._ck(self.L.gpc_hip_set_pipeline(self.h, int(lanes)))

    def pipeline_join(self):
        self._ck(self.L.gpc_hip_pipeline_join(self.h))

    def match_batch_device_packed(self, d_rawL, d_rawR, width, height, npairs, settings, d_packed, cap_per_pair,
                                  d_rows, d_counts, d_ncand=0):
        """Packed results (x | xR << 16 per support + per-row counts) left in HBM; epipolar sort-matcher only."""
        self._ck(self.L.gpc_hip_match_batch_device_packed(self.h, C.c_void_p(d_rawL), C.c_void_p(d_rawR), width, height,
                                                          npairs, C.byref(settings), C.c_void_p(d_packed), cap_per_pair,
                                                          C.c_void_p(d_rows), C.c_void_p(d_counts), C.c_void_p(d_ncand or 0)))

    # ---- frame sequences (optical flow): Forest::stereoMatch of every consecutive pair, each frame hashed once
    def match_sequence(self, frames, settings, cap=None):
        """frames: uint8 [N, H, W] in host memory (N >= 2) -> (records [N-1, cap] of CORR_DTYPE, true counts [N-1],
        candidate counts per frame [N], status).  Row t holds the first min(counts[t], cap) correspondences of the pair
        (frames[t], frames[t+1])."""
        frames = np.ascontiguousarray(frames, np.uint8)
        if frames.ndim != 3:
            raise ValueError("frames must be [N, H, W]")
        N, H, W = frames.shape
        cap = cap if cap is not None else W * H
        out = np.empty((max(N - 1, 1), max(cap, 1)), CORR_DTYPE)
        counts = np.zeros(max(N - 1, 1), np.int32)
        ncand = np.zeros(N, np.int32)
        st = self.L.gpc_hip_match_sequence(self.h, _ptr(frames), W, H, N, C.byref(settings), _ptr(out), cap,
                                           _ptr(counts), _ptr(ncand))
        self._ck(st, allow=(E_CAPACITY,))
        return out, counts, ncand, st

    def match_sequence_device(self, d_frames, width, height, nframes, settings, d_out, cap_per_pair, d_counts, d_ncand=0):
        """Frames [nframes][height][width] in HBM -> d_out[nframes-1][cap_per_pair] correspondences, d_counts[nframes-1],
        d_ncand[nframes] (optional); asynchronous as match_batch_device."""
        self._ck(self.L.gpc_hip_match_sequence_device(self.h, C.c_void_p(d_frames), width, height, nframes,
                                                      C.byref(settings), C.c_void_p(d_out), cap_per_pair,
                                                      C.c_void_p(d_counts), C.c_void_p(d_ncand or 0)))

    # ---- scoring against ground truth (gpc_hip_score_*): exact counts per pair, SCORE_DTYPE
    def _score_records_device(self, fn, d_records, cap_per_pair, d_counts, width, height, npairs, d_u, d_v, d_ignore,
                              thr, d_scores, flow):
        t = score_thresholds(thr)
        if not d_records or not d_counts or not d_scores or not d_u:
            raise ValueError("records, counts, scores and truth u: device pointers")
        if flow and not d_v:
            raise ValueError("truth: correspondences need v")
        if not flow and d_v:
            raise ValueError("truth: v must be 0 for supports")
        if int(cap_per_pair) <= 0 or int(npairs) <= 0 or int(width) <= 0 or int(height) <= 0:
            raise ValueError("cap_per_pair, npairs, width, height: positive")
        tr = Truth(d_u, d_v or None, d_ignore or None)
        self._ck(fn(self.h, C.c_void_p(d_records), int(cap_per_pair), C.c_void_p(d_counts), int(width), int(height),
                    int(npairs), C.byref(tr), _ptr(t), len(t), C.c_void_p(d_scores)))

    def score_supports_device(self, d_supports, cap_per_pair, d_counts, width, height, npairs, d_u, d_ignore, thr, d_scores):
        """Supports [npairs][cap_per_pair] already in HBM against disparity truth d_u [npairs][H][W] (float32) and an
        optional ignore mask (uint8) -> d_scores[npairs] (SCORE_DTYPE), asynchronous.  Pointers are integers."""
        self._score_records_device(self.L.gpc_hip_score_supports_device, d_supports, cap_per_pair, d_counts, width, height,
                                   npairs, d_u, 0, d_ignore, thr, d_scores, False)

    def score_correspondences_device(self, d_corr, cap_per_pair, d_counts, width, height, npairs, d_u, d_v, d_ignore, thr,
                                     d_scores):
        """Correspondences [npairs][cap_per_pair] in HBM against flow truth (d_u, d_v) -> d_scores[npairs]."""
        self._score_records_device(self.L.gpc_hip_score_correspondences_device, d_corr, cap_per_pair, d_counts, width,
                                   height, npairs, d_u, d_v, d_ignore, thr, d_scores, True)

    def score_batch_device(self, d_rawL, d_rawR, width, height, npairs, settings, d_u, d_ignore, thr, d_scores):
        """match_batch_device + scoring without the records leaving the library: d_scores[npairs], n_candidates and
        n_matchable filled."""
        t = score_thresholds(thr)
        if not d_rawL or not d_rawR or not d_u or not d_scores or int(npairs) <= 0:
            raise ValueError("images, truth u and scores: device pointers; npairs positive")
        tr = Truth(d_u, None, d_ignore or None)
        self._ck(self.L.gpc_hip_score_batch_device(self.h, C.c_void_p(d_rawL), C.c_void_p(d_rawR), int(width), int(height),
                                                   int(npairs), C.byref(settings), C.byref(tr), _ptr(t), len(t),
                                                   C.c_void_p(d_scores)))

    def score_sequence_device(self, d_frames, width, height, nframes, settings, d_u, d_v, d_ignore, thr, d_scores):
        """match_sequence_device + scoring: truth planes and d_scores have nframes - 1 entries."""
        t = score_thresholds(thr)
        if not d_frames or not d_u or not d_v or not d_scores or int(nframes) < 2:
            raise ValueError("frames, truth u, v and scores: device pointers; at least two frames")
        tr = Truth(d_u, d_v, d_ignore or None)
        self._ck(self.L.gpc_hip_score_sequence_device(self.h, C.c_void_p(d_frames), int(width), int(height), int(nframes),
                                                      C.byref(settings), C.byref(tr), _ptr(t), len(t), C.c_void_p(d_scores)))

    def score_records(self, records, counts, u, v, ignore, thr):
        """Host records [P, cap] (SUPPORT_DTYPE with v None, CORR_DTYPE with flow truth) and their true counts [P] against
        host truth planes [P, H, W] -> SCORE_DTYPE [P] (gpc_hip_score_supports / gpc_hip_score_correspondences)."""
        t = score_thresholds(thr)
        records = np.asarray(records)
        if records.dtype not in (SUPPORT_DTYPE, CORR_DTYPE) or records.ndim != 2 or records.shape[1] < 1:
            raise ValueError("records: [P, cap] of SUPPORT_DTYPE or CORR_DTYPE")
        flow = records.dtype == CORR_DTYPE
        records = np.ascontiguousarray(records)
        counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
        P, cap = records.shape
        uu = np.asarray(u) if u is not None else None
        if uu is None or uu.ndim != 3 or uu.shape[0] != P or len(counts) != P:
            raise ValueError("counts [P] and truth planes [P, H, W] for P = %d pairs" % P)
        u, v, ignore = _host_truth(u, v, ignore, uu.shape, flow)
        scores = np.zeros(P, SCORE_DTYPE)
        tr = Truth(u.ctypes.data, v.ctypes.data if flow else None, ignore.ctypes.data if ignore is not None else None)
        fn = self.L.gpc_hip_score_correspondences if flow else self.L.gpc_hip_score_supports
        self._ck(fn(self.h, _ptr(records), cap, _ptr(counts), uu.shape[2], uu.shape[1], P, C.byref(tr), _ptr(t), len(t),
                    _ptr(scores)))
        return scores

    def score_batch(self, rawL, rawR, settings, u, ignore, thr):
        """Host pairs [P, H, W] and host truth (u float32 [P, H, W], ignore uint8 [P, H, W] or None) -> SCORE_DTYPE [P]."""
        t = score_thresholds(thr)
        rawL, rawR = _host_frames(rawL), _host_frames(rawR)
        if rawL.ndim != 3 or rawL.shape != rawR.shape:
            raise ValueError("rawL / rawR: (P, H, W) arrays of one shape")
        P, H, W = rawL.shape
        u, _, ignore = _host_truth(u, None, ignore, rawL.shape, False)
        scores = np.zeros(P, SCORE_DTYPE)
        tr = Truth(u.ctypes.data, None, ignore.ctypes.data if ignore is not None else None)
        self._ck(self.L.gpc_hip_score_batch(self.h, _ptr(rawL), _ptr(rawR), W, H, P, C.byref(settings), C.byref(tr), _ptr(t),
                                            len(t), _ptr(scores)))
        return scores

    def score_sequence(self, frames, settings, u, v, ignore, thr):
        """Host frames [N, H, W] and host flow truth of the N - 1 consecutive pairs -> SCORE_DTYPE [N - 1]."""
        t = score_thresholds(thr)
        frames = _host_frames(frames)
        if frames.ndim != 3 or frames.shape[0] < 2:
            raise ValueError("frames: (N, H, W) with N >= 2")
        N, H, W = frames.shape
        u, v, ignore = _host_truth(u, v, ignore, (N - 1, H, W), True)
        scores = np.zeros(N - 1, SCORE_DTYPE)
        tr = Truth(u.ctypes.data, v.ctypes.data, ignore.ctypes.data if ignore is not None else None)
        self._ck(self.L.gpc_hip_score_sequence(self.h, _ptr(frames), W, H, N, C.byref(settings), C.byref(tr), _ptr(t), len(t),
                                               _ptr(scores)))
        return scores

    # ---- dense fields against ground truth (gpc_hip_score_fields*): exact counts per pair, the field scored where it lies
    def score_fields_device(self, d_field, channels, width, height, npairs, d_u, d_v, d_ignore, prm, d_scores, d_cls=0, d_err=0):
        """A field [npairs][channels][height][width] int32 and truth planes [npairs][height][width] (d_u, d_v float32; d_v 0 for
        a disparity; d_ignore and d_cls uint8, optional) already in HBM -> d_scores [npairs] of FieldScore (512 bytes each),
        d_err [npairs][height][width] uint16 (optional); asynchronous, no forest needed.  Pointers are integers."""
        tr = Truth(d_u or None, d_v or None, d_ignore or None)
        self._ck(self.L.gpc_hip_score_fields_device(self.h, C.c_void_p(d_field), int(channels), int(width), int(height), int(npairs),
                                                    C.byref(tr), C.byref(prm), C.c_void_p(d_cls or 0), C.c_void_p(d_scores),
                                                    C.c_void_p(d_err or 0)))

    def score_fields(self, field, u, v=None, ignore=None, prm=None, cls=None, want_err=False):
        """A host field [P, C, height, width] int32 against host truth planes [P, height, width] (u, v float32; v None for a
        disparity; ignore, cls uint8 or None) -> (a ctypes array of P FieldScore, err [P, height, width] uint16 or None)."""
        field = np.ascontiguousarray(field, np.int32)
        if field.ndim != 4 or field.shape[0] < 1:
            raise ValueError("field: [P, C, height, width] int32")
        P, Cn, H, W = field.shape
        plane = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
        u, v, ignore, cls = plane(u, np.float32), plane(v, np.float32), plane(ignore, np.uint8), plane(cls, np.uint8)
        for a in (u, v, ignore, cls):
            if a is not None and a.shape != (P, H, W):
                raise ValueError("truth, ignore, cls: [P, height, width]")
        prm = prm if prm is not None else FieldScorePrm()
        scores = (FieldScore * P)()
        err = np.empty((P, H, W), np.uint16) if want_err else None
        tr = Truth(*[a.ctypes.data if a is not None else None for a in (u, v, ignore)])
        self._ck(self.L.gpc_hip_score_fields(self.h, _ptr(field), Cn, W, H, P, C.byref(tr), C.byref(prm), _ptr(cls),
                                             C.cast(scores, C.c_void_p), _ptr(err)))
        return scores, err

    # ---- point tracks (gpc_hip_track_*): the records of consecutive pairs chained on the device
    def track_records_device(self, d_corr, cap_per_pair, d_counts, width, height, npairs, d_next, d_track_id, d_tracks,
                             track_cap, d_ntracks):
        """Correspondences [npairs][cap_per_pair] already in HBM (the layout match_sequence_device writes) -> d_next and
        d_track_id [npairs][cap_per_pair] int32, d_tracks [track_cap] of TRACK_DTYPE, d_ntracks [1] int32; asynchronous, no
        forest needed.  Pointers are integers."""
        self._ck(self.L.gpc_hip_track_records_device(self.h, C.c_void_p(d_corr), int(cap_per_pair), C.c_void_p(d_counts),
                                                     int(width), int(height), int(npairs), C.c_void_p(d_next),
                                                     C.c_void_p(d_track_id), C.c_void_p(d_tracks or 0), int(track_cap),
                                                     C.c_void_p(d_ntracks)))

    def track_sequence_device(self, d_frames, width, height, nframes, settings, d_corr, cap_per_pair, d_counts, d_ncand,
                              d_next, d_track_id, d_tracks, track_cap, d_ntracks):
        """match_sequence_device, then the links over what it wrote (gpc_hip_track_sequence_device)."""
        self._ck(self.L.gpc_hip_track_sequence_device(self.h, C.c_void_p(d_frames), int(width), int(height), int(nframes),
                                                      C.byref(settings), C.c_void_p(d_corr), int(cap_per_pair),
                                                      C.c_void_p(d_counts), C.c_void_p(d_ncand or 0), C.c_void_p(d_next),
                                                      C.c_void_p(d_track_id), C.c_void_p(d_tracks or 0), int(track_cap),
                                                      C.c_void_p(d_ntracks)))

    def track_records(self, records, counts, width, height, track_cap=None, next_out=None, id_out=None, tracks_out=None):
        """Host records [P, cap] of CORR_DTYPE and their true counts [P] -> (next [P, cap] int32, track_id [P, cap] int32,
        tracks [track_cap] of TRACK_DTYPE, n_tracks, status).  Entries of next / track_id beyond min(counts[t], cap) are
        left as they were (-1 in arrays made here).  track_cap None: one row per record slot, which always suffices."""
        records = np.asarray(records)
        if records.dtype != CORR_DTYPE or records.ndim != 2 or records.shape[1] < 1 or records.shape[0] < 1:
            raise ValueError("records: [P, cap] of CORR_DTYPE")
        if not records.flags.c_contiguous:
            records = np.ascontiguousarray(records)
        counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
        P, cap = records.shape
        if len(counts) != P:
            raise ValueError("counts: one per pair")
        track_cap = P * cap if track_cap is None else int(track_cap)
        nxt = next_out if next_out is not None else np.full((P, cap), -1, np.int32)
        tid = id_out if id_out is not None else np.full((P, cap), -1, np.int32)
        rows = tracks_out if tracks_out is not None else np.zeros(max(track_cap, 1), TRACK_DTYPE)
        n = C.c_int32(0)
        st = self.L.gpc_hip_track_records(self.h, _ptr(records), cap, _ptr(counts), int(width), int(height), P, _ptr(nxt),
                                          _ptr(tid), _ptr(rows), track_cap, C.byref(n))
        self._ck(st, allow=(E_CAPACITY,))
        return nxt, tid, rows[:min(n.value, track_cap)], n.value, st

    def track_sequence(self, frames, settings, cap=None, track_cap=None):
        """frames: uint8 [N, H, W] in host memory -> (records [N-1, cap], counts [N-1], candidates per frame [N],
        next [N-1, cap], track_id [N-1, cap], tracks, n_tracks, status): match_sequence plus the tracks of its records.
        The whole sequence is staged on the device (gpc_hip_track_sequence)."""
        frames = _host_frames(frames)
        if frames.ndim != 3 or frames.shape[0] < 2:
            raise ValueError("frames: (N, H, W) with N >= 2")
        N, H, W = frames.shape
        cap = cap if cap is not None else (W - 26) * (H - 26)
        track_cap = (N - 1) * cap if track_cap is None else int(track_cap)
        out = np.empty((N - 1, max(cap, 1)), CORR_DTYPE)
        counts = np.zeros(N - 1, np.int32)
        ncand = np.zeros(N, np.int32)
        nxt = np.full((N - 1, max(cap, 1)), -1, np.int32)
        tid = np.full((N - 1, max(cap, 1)), -1, np.int32)
        rows = np.zeros(max(track_cap, 1), TRACK_DTYPE)
        n = C.c_int32(0)
        st = self.L.gpc_hip_track_sequence(self.h, _ptr(frames), W, H, N, C.byref(settings), _ptr(out), cap, _ptr(counts),
                                           _ptr(ncand), _ptr(nxt), _ptr(tid), _ptr(rows), track_cap, C.byref(n))
        self._ck(st, allow=(E_CAPACITY,))
        return out, counts, ncand, nxt, tid, rows[:min(n.value, track_cap)], n.value, st

    def track_stream(self, width, height, settings, cap_per_pair, track_cap):
        """A TrackStream of this context (gpc_hip_track_stream_create): frames or records pushed as they arrive, track ids
        kept across pushes.  settings None: a stream that is only given records."""
        return TrackStream(self, width, height, settings, cap_per_pair, track_cap)

    # ---- match filtering (gpc_hip_consensus_*): grid motion consensus over a pair's records
    def consensus_records_device(self, d_rec, corr, cap_per_pair, d_counts, width, height, npairs, prm, d_keep, d_out, cap_out,
                                 d_index, d_out_counts):
        """Records [npairs][cap_per_pair] already in HBM (corr: CORR_DTYPE, else SUPPORT_DTYPE) -> d_keep [npairs][cap_per_pair]
        uint8 (optional), d_out [npairs][cap_out] kept records in input order, d_index [npairs][cap_out] int32 (optional),
        d_out_counts [npairs] int32; asynchronous, no forest needed.  Pointers are integers."""
        fn = self.L.gpc_hip_consensus_correspondences_device if corr else self.L.gpc_hip_consensus_supports_device
        self._ck(fn(self.h, C.c_void_p(d_rec), int(cap_per_pair), C.c_void_p(d_counts), int(width), int(height), int(npairs),
                    C.byref(prm), C.c_void_p(d_keep or 0), C.c_void_p(d_out), int(cap_out), C.c_void_p(d_index or 0),
                    C.c_void_p(d_out_counts)))

    def consensus_batch_device(self, d_rawL, d_rawR, width, height, npairs, settings, prm, d_out, cap_out, d_out_counts,
                               d_raw_counts=0, d_ncand=0):
        """match_batch_device into the context's every-record workspace, then the filter: d_out [npairs][cap_out] supports."""
        self._ck(self.L.gpc_hip_consensus_batch_device(self.h, C.c_void_p(d_rawL), C.c_void_p(d_rawR), int(width), int(height),
                                                       int(npairs), C.byref(settings), C.byref(prm), C.c_void_p(d_out),
                                                       int(cap_out), C.c_void_p(d_out_counts), C.c_void_p(d_raw_counts or 0),
                                                       C.c_void_p(d_ncand or 0)))

    def consensus_sequence_device(self, d_frames, width, height, nframes, settings, prm, d_out, cap_out, d_out_counts,
                                  d_raw_counts=0, d_ncand=0):
        """match_sequence_device, then the filter: d_out [nframes-1][cap_out] correspondences."""
        self._ck(self.L.gpc_hip_consensus_sequence_device(self.h, C.c_void_p(d_frames), int(width), int(height), int(nframes),
                                                          C.byref(settings), C.byref(prm), C.c_void_p(d_out), int(cap_out),
                                                          C.c_void_p(d_out_counts), C.c_void_p(d_raw_counts or 0),
                                                          C.c_void_p(d_ncand or 0)))

    def consensus_records(self, records, counts, width, height, prm=None, cap_out=None, keep=None, out=None, index=None):
        """Host records [P, cap] (SUPPORT_DTYPE or CORR_DTYPE) and their true counts [P] -> (keep [P, cap] uint8, out
        [P, cap_out], index [P, cap_out] int32, out_counts [P], status).  Entries the filter does not write are left as
        they were (0 / -1 in arrays made here); status is E_CAPACITY when a pair keeps more than cap_out records."""
        records = np.asarray(records)
        if records.dtype not in (SUPPORT_DTYPE, CORR_DTYPE) or records.ndim != 2 or records.shape[1] < 1 or records.shape[0] < 1:
            raise ValueError("records: [P, cap] of SUPPORT_DTYPE or CORR_DTYPE")
        corr = records.dtype == CORR_DTYPE
        if not records.flags.c_contiguous:
            records = np.ascontiguousarray(records)
        counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
        P, cap = records.shape
        if len(counts) != P:
            raise ValueError("counts: one per pair")
        prm = prm if prm is not None else Consensus()
        cap_out = cap if cap_out is None else int(cap_out)
        keep = keep if keep is not None else np.zeros((P, cap), np.uint8)
        out = out if out is not None else np.zeros((P, max(cap_out, 1)), records.dtype)
        index = index if index is not None else np.full((P, max(cap_out, 1)), -1, np.int32)
        out_counts = np.zeros(P, np.int32)
        fn = self.L.gpc_hip_consensus_correspondences if corr else self.L.gpc_hip_consensus_supports
        st = fn(self.h, _ptr(records), cap, _ptr(counts), int(width), int(height), P, C.byref(prm), _ptr(keep), _ptr(out), cap_out,
                _ptr(index), _ptr(out_counts))
        self._ck(st, allow=(E_CAPACITY,))
        return keep, out, index, out_counts, st

    # ---- match refinement (gpc_hip_refine_*): sub-pixel position and photometric cost of every record
    def refine_records_device(self, d_rec, corr, cap_per_pair, d_counts, d_imgL, d_imgR, width, height, npairs, radius, d_ref,
                              d_out=0):
        """Records [npairs][cap_per_pair] (corr: CORR_DTYPE, else SUPPORT_DTYPE) and 8-bit images [npairs][height][width]
        already in HBM -> d_ref [npairs][cap_per_pair] of REFINEMENT_DTYPE and, for supports, d_out (optional) the records with
        the refined d; asynchronous, no forest needed.  Pointers are integers."""
        if corr:
            if d_out:
                raise ValueError("d_out: supports only")
            self._ck(self.L.gpc_hip_refine_correspondences_device(
                self.h, C.c_void_p(d_rec), int(cap_per_pair), C.c_void_p(d_counts), C.c_void_p(d_imgL), C.c_void_p(d_imgR),
                int(width), int(height), int(npairs), int(radius), C.c_void_p(d_ref)))
        else:
            self._ck(self.L.gpc_hip_refine_supports_device(
                self.h, C.c_void_p(d_rec), int(cap_per_pair), C.c_void_p(d_counts), C.c_void_p(d_imgL), C.c_void_p(d_imgR),
                int(width), int(height), int(npairs), int(radius), C.c_void_p(d_ref), C.c_void_p(d_out or 0)))

    def refine_batch_device(self, d_rawL, d_rawR, width, height, npairs, settings, radius, d_supports, cap_per_pair, d_counts,
                            d_ncand, d_ref, d_out=0):
        """match_batch_device into d_supports / d_counts / d_ncand, then the refinement of what it wrote over the raw images."""
        self._ck(self.L.gpc_hip_refine_batch_device(self.h, C.c_void_p(d_rawL), C.c_void_p(d_rawR), int(width), int(height),
                                                    int(npairs), C.byref(settings), int(radius), C.c_void_p(d_supports),
                                                    int(cap_per_pair), C.c_void_p(d_counts), C.c_void_p(d_ncand or 0),
                                                    C.c_void_p(d_ref), C.c_void_p(d_out or 0)))

    def refine_sequence_device(self, d_frames, width, height, nframes, settings, radius, d_corr, cap_per_pair, d_counts, d_ncand,
                               d_ref):
        """match_sequence_device into d_corr / d_counts / d_ncand, then the refinement over frames t and t + 1."""
        self._ck(self.L.gpc_hip_refine_sequence_device(self.h, C.c_void_p(d_frames), int(width), int(height), int(nframes),
                                                       C.byref(settings), int(radius), C.c_void_p(d_corr), int(cap_per_pair),
                                                       C.c_void_p(d_counts), C.c_void_p(d_ncand or 0), C.c_void_p(d_ref)))

    def refine_records(self, records, counts, imgL, imgR, radius=3, ref=None, out=None):
        """Host records [P, cap] (SUPPORT_DTYPE or CORR_DTYPE), their true counts [P] and host images [P, H, W] uint8 ->
        (ref [P, cap] of REFINEMENT_DTYPE, out [P, cap] supports with the refined d, or None for correspondences).  Entries
        beyond min(counts[t], cap) are left as they were (zero in arrays made here)."""
        records = np.asarray(records)
        if records.dtype not in (SUPPORT_DTYPE, CORR_DTYPE) or records.ndim != 2 or records.shape[1] < 1 or records.shape[0] < 1:
            raise ValueError("records: [P, cap] of SUPPORT_DTYPE or CORR_DTYPE")
        corr = records.dtype == CORR_DTYPE
        if not records.flags.c_contiguous:
            records = np.ascontiguousarray(records)
        counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
        imgL, imgR = _host_frames(imgL), _host_frames(imgR)
        P, cap = records.shape
        if imgL.ndim != 3 or imgL.shape != imgR.shape or imgL.shape[0] != P or len(counts) != P:
            raise ValueError("counts [P] and images [P, H, W] of one shape for P = %d pairs" % P)
        _, H, W = imgL.shape
        ref = ref if ref is not None else np.zeros((P, cap), REFINEMENT_DTYPE)
        if corr:
            if out is not None:
                raise ValueError("out: supports only")
            self._ck(self.L.gpc_hip_refine_correspondences(self.h, _ptr(records), cap, _ptr(counts), _ptr(imgL), _ptr(imgR), W, H, P,
                                                           int(radius), _ptr(ref)))
            return ref, None
        out = out if out is not None else np.zeros((P, cap), SUPPORT_DTYPE)
        self._ck(self.L.gpc_hip_refine_supports(self.h, _ptr(records), cap, _ptr(counts), _ptr(imgL), _ptr(imgR), W, H, P,
                                                int(radius), _ptr(ref), _ptr(out)))
        return ref, out

    # ---- matching over an image pyramid (gpc_hip_pyramid_*): per-level matches merged on the device
    def pyramid_down_device(self, d_src, width, height, nimages, d_dst):
        """One 2x2-mean step over [nimages][height][width] bytes in HBM -> [nimages][height // 2][width // 2]; asynchronous."""
        self._ck(self.L.gpc_hip_pyramid_down_device(self.h, C.c_void_p(d_src), int(width), int(height), int(nimages),
                                                    C.c_void_p(d_dst)))

    def pyramid_merge_device(self, d_rec, caps, d_cnt, corr, width, height, npairs, d_out, cap_per_pair, d_counts,
                             d_level_counts):
        """The merge alone: d_rec[l], caps[l], d_cnt[l] are level l's unmapped records [npairs][caps[l]] (corr: CORR_DTYPE,
        else SUPPORT_DTYPE) and counts [npairs] in HBM -> d_out[npairs][cap_per_pair] in level 0's coordinates, d_counts
        [npairs], d_level_counts [levels][npairs]; asynchronous, no forest needed.  Pointers are integers."""
        levels = len(d_rec)
        if not (len(caps) == len(d_cnt) == levels):
            raise ValueError("d_rec, caps, d_cnt: one entry per level")
        recs = (C.c_void_p * levels)(*[C.c_void_p(int(p)) for p in d_rec])
        cnts = (C.c_void_p * levels)(*[C.c_void_p(int(p)) for p in d_cnt])
        cap_arr = (C.c_int32 * levels)(*[int(v) for v in caps])
        fn = self.L.gpc_hip_pyramid_merge_correspondences_device if corr else self.L.gpc_hip_pyramid_merge_supports_device
        self._ck(fn(self.h, C.cast(recs, C.c_void_p), C.cast(cap_arr, C.c_void_p), C.cast(cnts, C.c_void_p), int(width),
                    int(height), int(npairs), levels, C.c_void_p(d_out), int(cap_per_pair), C.c_void_p(d_counts),
                    C.c_void_p(d_level_counts)))

    def pyramid_batch_device(self, d_rawL, d_rawR, width, height, npairs, levels, settings, d_out, cap_per_pair, d_counts,
                             d_level_counts, d_ncand=0):
        """match_batch_device on every level of the pairs' pyramids, merged: d_out[npairs][cap_per_pair] supports in level 0's
        coordinates, d_counts[npairs], d_level_counts[levels][npairs], d_ncand[levels][npairs][2] (optional)."""
        self._ck(self.L.gpc_hip_pyramid_batch_device(self.h, C.c_void_p(d_rawL), C.c_void_p(d_rawR), int(width), int(height),
                                                     int(npairs), int(levels), C.byref(settings), C.c_void_p(d_out),
                                                     int(cap_per_pair), C.c_void_p(d_counts), C.c_void_p(d_level_counts),
                                                     C.c_void_p(d_ncand or 0)))

    def pyramid_sequence_device(self, d_frames, width, height, nframes, levels, settings, d_out, cap_per_pair, d_counts,
                                d_level_counts, d_ncand=0):
        """match_sequence_device on every level, merged: d_out[nframes-1][cap_per_pair] correspondences, d_counts[nframes-1],
        d_level_counts[levels][nframes-1], d_ncand[levels][nframes] (optional)."""
        self._ck(self.L.gpc_hip_pyramid_sequence_device(self.h, C.c_void_p(d_frames), int(width), int(height), int(nframes),
                                                        int(levels), C.byref(settings), C.c_void_p(d_out), int(cap_per_pair),
                                                        C.c_void_p(d_counts), C.c_void_p(d_level_counts),
                                                        C.c_void_p(d_ncand or 0)))

    def pyramid_batch(self, rawL, rawR, levels, settings, cap, out=None):
        """Host pairs [P, H, W] uint8 (pageable or page-locked) -> (supports [P, cap], counts [P], level_counts [levels, P],
        ncand [levels, P, 2], status).  `out` is written only as far as each pair's records go."""
        rawL, rawR = _host_frames(rawL), _host_frames(rawR)
        if rawL.ndim != 3 or rawL.shape != rawR.shape:
            raise ValueError("rawL, rawR: [P, H, W] of one shape")
        P, H, W = rawL.shape
        out = out if out is not None else np.zeros((P, cap), SUPPORT_DTYPE)
        counts, lc, ncand = np.zeros(P, np.int32), np.zeros((levels, P), np.int32), np.zeros((levels, P, 2), np.int32)
        st = self.L.gpc_hip_pyramid_batch(self.h, _ptr(rawL), _ptr(rawR), W, H, P, int(levels), C.byref(settings), _ptr(out),
                                          int(cap), _ptr(counts), _ptr(lc), _ptr(ncand))
        self._ck(st, allow=(E_CAPACITY,))
        return out, counts, lc, ncand, st

    def pyramid_sequence(self, frames, levels, settings, cap, out=None):
        """Host frames [N, H, W] uint8 -> (correspondences [N-1, cap], counts [N-1], level_counts [levels, N-1], ncand
        [levels, N], status)."""
        frames = _host_frames(frames)
        if frames.ndim != 3 or frames.shape[0] < 2:
            raise ValueError("frames: [N, H, W], N >= 2")
        N, H, W = frames.shape
        out = out if out is not None else np.zeros((N - 1, cap), CORR_DTYPE)
        counts, lc, ncand = np.zeros(N - 1, np.int32), np.zeros((levels, N - 1), np.int32), np.zeros((levels, N), np.int32)
        st = self.L.gpc_hip_pyramid_sequence(self.h, _ptr(frames), W, H, N, int(levels), C.byref(settings), _ptr(out), int(cap),
                                             _ptr(counts), _ptr(lc), _ptr(ncand))
        self._ck(st, allow=(E_CAPACITY,))
        return out, counts, lc, ncand, st

    # ---- dense maps from sparse matches (gpc_hip_densify_*): the hierarchical fill
    def densify_records_device(self, d_rec, corr, cap_per_pair, d_counts, width, height, npairs, prm, d_value, d_level=0, d_ref=0):
        """Records [npairs][cap_per_pair] already in HBM (corr: CORR_DTYPE, else SUPPORT_DTYPE), optionally their refinements
        d_ref [npairs][cap_per_pair] of REFINEMENT_DTYPE -> d_value [npairs][C][height][width] int32 in 1/256 pixel (C = 2 for
        correspondences, else 1; DENSE_NONE where nothing fills the pixel), d_level [npairs][height][width] uint8 (optional);
        asynchronous, no forest needed.  Pointers are integers."""
        fn = self.L.gpc_hip_densify_correspondences_device if corr else self.L.gpc_hip_densify_supports_device
        self._ck(fn(self.h, C.c_void_p(d_rec), int(cap_per_pair), C.c_void_p(d_counts), C.c_void_p(d_ref or 0), int(width),
                    int(height), int(npairs), C.byref(prm), C.c_void_p(d_value), C.c_void_p(d_level or 0)))

    def densify_batch_device(self, d_rawL, d_rawR, width, height, npairs, settings, prm, d_value, d_level=0, refine_radius=0,
                             d_counts=0, d_ncand=0):
        """match_batch_device into the context's every-record workspace, the refinement over the raw images when
        refine_radius >= 1, then the fill: d_value [npairs][1][height][width], d_level [npairs][height][width]."""
        self._ck(self.L.gpc_hip_densify_batch_device(self.h, C.c_void_p(d_rawL), C.c_void_p(d_rawR), int(width), int(height),
                                                     int(npairs), C.byref(settings), int(refine_radius), C.byref(prm),
                                                     C.c_void_p(d_value), C.c_void_p(d_level or 0), C.c_void_p(d_counts or 0),
                                                     C.c_void_p(d_ncand or 0)))

    def densify_sequence_device(self, d_frames, width, height, nframes, settings, prm, d_value, d_level=0, refine_radius=0,
                                d_counts=0, d_ncand=0):
        """match_sequence_device, the refinement when refine_radius >= 1, then the fill: d_value [nframes-1][2][height][width]
        (u plane, v plane), d_level [nframes-1][height][width]."""
        self._ck(self.L.gpc_hip_densify_sequence_device(self.h, C.c_void_p(d_frames), int(width), int(height), int(nframes),
                                                        C.byref(settings), int(refine_radius), C.byref(prm), C.c_void_p(d_value),
                                                        C.c_void_p(d_level or 0), C.c_void_p(d_counts or 0),
                                                        C.c_void_p(d_ncand or 0)))

    def densify_records(self, records, counts, width, height, prm=None, ref=None, want_level=True):
        """Host records [P, cap] (SUPPORT_DTYPE or CORR_DTYPE), their true counts [P] and optionally their refinements
        [P, cap] of REFINEMENT_DTYPE -> (value [P, C, height, width] int32, level [P, height, width] uint8 or None)."""
        records = np.asarray(records)
        if records.dtype not in (SUPPORT_DTYPE, CORR_DTYPE) or records.ndim != 2 or records.shape[1] < 1 or records.shape[0] < 1:
            raise ValueError("records: [P, cap] of SUPPORT_DTYPE or CORR_DTYPE")
        corr = records.dtype == CORR_DTYPE
        if not records.flags.c_contiguous:
            records = np.ascontiguousarray(records)
        counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
        P, cap = records.shape
        if len(counts) != P:
            raise ValueError("counts: one per pair")
        if ref is not None:
            ref = np.ascontiguousarray(ref)
            if ref.dtype != REFINEMENT_DTYPE or ref.shape != records.shape:
                raise ValueError("ref: [P, cap] of REFINEMENT_DTYPE")
        prm = prm if prm is not None else Densify()
        width, height = int(width), int(height)
        value = np.empty((P, 2 if corr else 1, max(height, 1), max(width, 1)), np.int32)
        level = np.empty((P, max(height, 1), max(width, 1)), np.uint8) if want_level else None
        fn = self.L.gpc_hip_densify_correspondences if corr else self.L.gpc_hip_densify_supports
        self._ck(fn(self.h, _ptr(records), cap, _ptr(counts), _ptr(ref), width, height, P, C.byref(prm), _ptr(value), _ptr(level)))
        return value, level

    # ---- clean dense fields (gpc_hip_clean_*): cross-check, speckles, median
    def clean_fields_device(self, d_fwd, channels, width, height, npairs, prm, d_out, d_bwd=0, d_state=0, d_label=0, d_stats=0):
        """Fields [npairs][channels][height][width] int32 already in HBM, as the densify calls write them (d_bwd: the field of
        the reversed records, needed when prm.check_tol_q8 >= 0) -> d_out of the same shape (DENSE_NONE where the pixel is not
        kept), d_state [npairs][height][width] uint8, d_label [npairs][height][width] int32, d_stats [npairs][4] int32 (all
        optional); asynchronous, no forest needed.  Pointers are integers."""
        self._ck(self.L.gpc_hip_clean_fields_device(self.h, C.c_void_p(d_fwd), C.c_void_p(d_bwd or 0), int(channels), int(width),
                                                    int(height), int(npairs), C.byref(prm), C.c_void_p(d_out), C.c_void_p(d_state or 0),
                                                    C.c_void_p(d_label or 0), C.c_void_p(d_stats or 0)))

    def flip_records_device(self, d_rec, corr, cap_per_pair, d_counts, npairs, d_rec_out, d_ref=0, d_ref_out=0):
        """Records [npairs][cap_per_pair] in HBM (corr: CORR_DTYPE, else SUPPORT_DTYPE) read from their target's side, slot i to
        slot i as far as the counts go; d_ref / d_ref_out: their refinements, shifts negated (both or neither).  In place is
        allowed (d_rec_out == d_rec, d_ref_out == d_ref)."""
        fn = self.L.gpc_hip_flip_correspondences_device if corr else self.L.gpc_hip_flip_supports_device
        self._ck(fn(self.h, C.c_void_p(d_rec), C.c_void_p(d_ref or 0), int(cap_per_pair), C.c_void_p(d_counts), int(npairs),
                    C.c_void_p(d_rec_out), C.c_void_p(d_ref_out or 0)))

    def clean_batch_device(self, d_rawL, d_rawR, width, height, npairs, settings, fill, prm, d_out, d_state=0, d_label=0, d_stats=0,
                           d_fwd=0, d_level=0, refine_radius=0, d_counts=0, d_ncand=0):
        """densify_batch_device (its field is the forward field, d_fwd / d_level optional), the records reversed and filled
        again, then clean_fields_device: d_out [npairs][1][height][width]."""
        self._ck(self.L.gpc_hip_clean_batch_device(self.h, C.c_void_p(d_rawL), C.c_void_p(d_rawR), int(width), int(height), int(npairs),
                                                   C.byref(settings), int(refine_radius), C.byref(fill), C.byref(prm),
                                                   C.c_void_p(d_out), C.c_void_p(d_state or 0), C.c_void_p(d_label or 0),
                                                   C.c_void_p(d_stats or 0), C.c_void_p(d_fwd or 0), C.c_void_p(d_level or 0),
                                                   C.c_void_p(d_counts or 0), C.c_void_p(d_ncand or 0)))

    def clean_sequence_device(self, d_frames, width, height, nframes, settings, fill, prm, d_out, d_state=0, d_label=0, d_stats=0,
                              d_fwd=0, d_level=0, refine_radius=0, d_counts=0, d_ncand=0):
        """densify_sequence_device, the records reversed and filled again, then clean_fields_device: d_out
        [nframes-1][2][height][width]."""
        self._ck(self.L.gpc_hip_clean_sequence_device(self.h, C.c_void_p(d_frames), int(width), int(height), int(nframes),
                                                      C.byref(settings), int(refine_radius), C.byref(fill), C.byref(prm),
                                                      C.c_void_p(d_out), C.c_void_p(d_state or 0), C.c_void_p(d_label or 0),
                                                      C.c_void_p(d_stats or 0), C.c_void_p(d_fwd or 0), C.c_void_p(d_level or 0),
                                                      C.c_void_p(d_counts or 0), C.c_void_p(d_ncand or 0)))

    def clean_fields(self, fwd, bwd=None, prm=None, want_state=True, want_label=True, want_stats=True):
        """Host fields [P, C, height, width] int32 (bwd optional: prm.check_tol_q8 must then be -1) -> (out [P, C, height,
        width] int32, state [P, height, width] uint8, label [P, height, width] int32, stats [P, 4] int32; None where not
        wanted)."""
        fwd = np.ascontiguousarray(fwd, np.int32)
        if fwd.ndim != 4 or fwd.shape[0] < 1:
            raise ValueError("fwd: [P, C, height, width] int32")
        if bwd is not None:
            bwd = np.ascontiguousarray(bwd, np.int32)
            if bwd.shape != fwd.shape:
                raise ValueError("bwd: the shape of fwd")
        prm = prm if prm is not None else Clean()
        P, Cn, H, W = fwd.shape
        out = np.empty(fwd.shape, np.int32)
        state = np.empty((P, H, W), np.uint8) if want_state else None
        label = np.empty((P, H, W), np.int32) if want_label else None
        stats = np.empty((P, 4), np.int32) if want_stats else None
        self._ck(self.L.gpc_hip_clean_fields(self.h, _ptr(fwd), _ptr(bwd), Cn, W, H, P, C.byref(prm), _ptr(out), _ptr(state),
                                             _ptr(label), _ptr(stats)))
        return out, state, label, stats

    # ---- search the image pair around every pixel of a field (gpc_hip_search_*): the filled value is the prior
    def search_fields_device(self, d_field, d_imgL, d_imgR, channels, width, height, npairs, prm, d_out, d_cost=0, d_choice=0, d_stats=0):
        """A field [npairs][channels][height][width] int32 and the images [npairs][height][width] uint8 already in HBM -> d_out
        of the field's shape (it may be d_field itself), d_cost [npairs][height][width] uint16, d_choice [npairs][height][width]
        uint8, d_stats [npairs][4] int32 (all optional); asynchronous, no forest needed.  Pointers are integers."""
        self._ck(self.L.gpc_hip_search_fields_device(self.h, C.c_void_p(d_field), C.c_void_p(d_imgL), C.c_void_p(d_imgR), int(channels),
                                                     int(width), int(height), int(npairs), C.byref(prm), C.c_void_p(d_out),
                                                     C.c_void_p(d_cost or 0), C.c_void_p(d_choice or 0), C.c_void_p(d_stats or 0)))

    def search_batch_device(self, d_rawL, d_rawR, width, height, npairs, settings, fill, search, prm, d_out, d_state=0, d_label=0,
                            d_stats=0, d_fwd=0, d_level=0, refine_radius=0, d_counts=0, d_ncand=0, d_cost=0):
        """clean_batch_device with search_fields_device run in place over the forward field (d_fwd, its costs d_cost) and, with
        the images exchanged, over the backward field: d_out [npairs][1][height][width]."""
        self._ck(self.L.gpc_hip_search_batch_device(self.h, C.c_void_p(d_rawL), C.c_void_p(d_rawR), int(width), int(height), int(npairs),
                                                    C.byref(settings), int(refine_radius), C.byref(fill), C.byref(search), C.byref(prm),
                                                    C.c_void_p(d_out), C.c_void_p(d_state or 0), C.c_void_p(d_label or 0),
                                                    C.c_void_p(d_stats or 0), C.c_void_p(d_fwd or 0), C.c_void_p(d_level or 0),
                                                    C.c_void_p(d_counts or 0), C.c_void_p(d_ncand or 0), C.c_void_p(d_cost or 0)))

    def search_sequence_device(self, d_frames, width, height, nframes, settings, fill, search, prm, d_out, d_state=0, d_label=0,
                               d_stats=0, d_fwd=0, d_level=0, refine_radius=0, d_counts=0, d_ncand=0, d_cost=0):
        """clean_sequence_device with the search over frames t and t + 1 behind each fill: d_out [nframes-1][2][height][width]."""
        self._ck(self.L.gpc_hip_search_sequence_device(self.h, C.c_void_p(d_frames), int(width), int(height), int(nframes),
                                                       C.byref(settings), int(refine_radius), C.byref(fill), C.byref(search),
                                                       C.byref(prm), C.c_void_p(d_out), C.c_void_p(d_state or 0),
                                                       C.c_void_p(d_label or 0), C.c_void_p(d_stats or 0), C.c_void_p(d_fwd or 0),
                                                       C.c_void_p(d_level or 0), C.c_void_p(d_counts or 0), C.c_void_p(d_ncand or 0),
                                                       C.c_void_p(d_cost or 0)))

    def search_fields(self, field, imgL, imgR, prm=None, want_cost=True, want_choice=True, want_stats=True):
        """A host field [P, C, height, width] int32 and images [P, height, width] uint8 -> (out [P, C, height, width] int32, cost
        [P, height, width] uint16, choice [P, height, width] uint8, stats [P, 4] int32; None where not wanted)."""
        field = np.ascontiguousarray(field, np.int32)
        imgL, imgR = np.ascontiguousarray(imgL, np.uint8), np.ascontiguousarray(imgR, np.uint8)
        if field.ndim != 4 or field.shape[0] < 1:
            raise ValueError("field: [P, C, height, width] int32")
        P, Cn, H, W = field.shape
        if imgL.shape != (P, H, W) or imgR.shape != (P, H, W):
            raise ValueError("imgL, imgR: [P, height, width] uint8")
        prm = prm if prm is not None else Search()
        out = np.empty(field.shape, np.int32)
        cost = np.empty((P, H, W), np.uint16) if want_cost else None
        choice = np.empty((P, H, W), np.uint8) if want_choice else None
        stats = np.empty((P, 4), np.int32) if want_stats else None
        self._ck(self.L.gpc_hip_search_fields(self.h, _ptr(field), _ptr(imgL), _ptr(imgR), Cn, W, H, P, C.byref(prm), _ptr(out),
                                              _ptr(cost), _ptr(choice), _ptr(stats)))
        return out, cost, choice, stats

    # ---- propagate field values between neighbours (gpc_hip_propagate_*): between the fill and the search
    def propagate_fields_device(self, d_field, d_imgL, d_imgR, channels, width, height, npairs, prm, d_out, d_cost=0, d_choice=0,
                                d_stats=0):
        """A field [npairs][channels][height][width] int32 and the images [npairs][height][width] uint8 already in HBM -> d_out
        of the field's shape (it may be d_field itself), d_cost [npairs][height][width] uint16 and d_choice
        [npairs][height][width] uint8 of the last iteration, d_stats [npairs][iterations][4] int32 (all optional);
        asynchronous, no forest needed.  Pointers are integers."""
        self._ck(self.L.gpc_hip_propagate_fields_device(self.h, C.c_void_p(d_field), C.c_void_p(d_imgL), C.c_void_p(d_imgR), int(channels),
                                                        int(width), int(height), int(npairs), C.byref(prm), C.c_void_p(d_out),
                                                        C.c_void_p(d_cost or 0), C.c_void_p(d_choice or 0), C.c_void_p(d_stats or 0)))

    def propagate_fields(self, field, imgL, imgR, prm=None, want_cost=True, want_choice=True, want_stats=True):
        """A host field [P, C, height, width] int32 and images [P, height, width] uint8 -> (out [P, C, height, width] int32, cost
        [P, height, width] uint16, choice [P, height, width] uint8, stats [P, iterations, 4] int32; None where not wanted)."""
        field = np.ascontiguousarray(field, np.int32)
        imgL, imgR = np.ascontiguousarray(imgL, np.uint8), np.ascontiguousarray(imgR, np.uint8)
        if field.ndim != 4 or field.shape[0] < 1:
            raise ValueError("field: [P, C, height, width] int32")
        P, Cn, H, W = field.shape
        if imgL.shape != (P, H, W) or imgR.shape != (P, H, W):
            raise ValueError("imgL, imgR: [P, height, width] uint8")
        prm = prm if prm is not None else Propagate()
        out = np.empty(field.shape, np.int32)
        cost = np.empty((P, H, W), np.uint16) if want_cost else None
        choice = np.empty((P, H, W), np.uint8) if want_choice else None
        stats = np.empty((P, max(1, int(prm.iterations)), 4), np.int32) if want_stats else None
        self._ck(self.L.gpc_hip_propagate_fields(self.h, _ptr(field), _ptr(imgL), _ptr(imgR), Cn, W, H, P, C.byref(prm), _ptr(out),
                                                 _ptr(cost), _ptr(choice), _ptr(stats)))
        return out, cost, choice, stats

    # ---- close holes along scanlines from the background side (gpc_hip_gapfill_*): between the cleaner and the completion
    def gapfill_fields_device(self, d_field, d_guide, channels, width, height, npairs, prm, d_out, d_how=0, d_stats=0):
        """A field [npairs][channels][height][width] int32 and (required with select = 1, else it may be 0) a guide
        [npairs][height][width] uint8 already in HBM -> d_out of the field's shape (it may be d_field itself), d_how
        [npairs][height][width] uint8, d_stats [npairs][4] int32 (both optional); asynchronous, no forest needed.  Pointers
        are integers."""
        self._ck(self.L.gpc_hip_gapfill_fields_device(self.h, C.c_void_p(d_field), C.c_void_p(d_guide or 0), int(channels), int(width),
                                                      int(height), int(npairs), C.byref(prm), C.c_void_p(d_out), C.c_void_p(d_how or 0),
                                                      C.c_void_p(d_stats or 0)))

    def gapfill_fields(self, field, guide=None, prm=None, want_how=True, want_stats=True):
        """A host field [P, C, height, width] int32 and optionally a guide [P, height, width] uint8 -> (out [P, C, height,
        width] int32, how [P, height, width] uint8, stats [P, 4] int32; None where not wanted)."""
        field = np.ascontiguousarray(field, np.int32)
        if field.ndim != 4 or field.shape[0] < 1:
            raise ValueError("field: [P, C, height, width] int32")
        P, Cn, H, W = field.shape
        if guide is not None:
            guide = np.ascontiguousarray(guide, np.uint8)
            if guide.shape != (P, H, W):
                raise ValueError("guide: [P, height, width] uint8")
        prm = prm if prm is not None else Gapfill()
        out = np.empty(field.shape, np.int32)
        how = np.empty((P, H, W), np.uint8) if want_how else None
        stats = np.empty((P, 4), np.int32) if want_stats else None
        self._ck(self.L.gpc_hip_gapfill_fields(self.h, _ptr(field), _ptr(guide), Cn, W, H, P, C.byref(prm), _ptr(out), _ptr(how),
                                               _ptr(stats)))
        return out, how, stats

    # ---- aggregate the search's costs along scanlines (gpc_hip_aggregate_*): the search's candidates, chosen with a smoothness term
    def aggregate_fields_device(self, d_field, d_imgL, d_imgR, channels, width, height, npairs, prm, d_out, d_cost=0, d_choice=0,
                                d_stats=0, d_agg=0):
        """search_fields_device with the choice made over the aggregated costs; d_agg [npairs][height][width] uint32 (optional)
        receives the best candidate's sum.  Asynchronous, no forest needed.  Pointers are integers."""
        self._ck(self.L.gpc_hip_aggregate_fields_device(self.h, C.c_void_p(d_field), C.c_void_p(d_imgL), C.c_void_p(d_imgR), int(channels),
                                                        int(width), int(height), int(npairs), C.byref(prm), C.c_void_p(d_out),
                                                        C.c_void_p(d_cost or 0), C.c_void_p(d_choice or 0), C.c_void_p(d_stats or 0),
                                                        C.c_void_p(d_agg or 0)))

    def aggregate_batch_device(self, d_rawL, d_rawR, width, height, npairs, settings, fill, aggregate, prm, d_out, d_state=0, d_label=0,
                               d_stats=0, d_fwd=0, d_level=0, refine_radius=0, d_counts=0, d_ncand=0, d_cost=0):
        """search_batch_device with aggregate_fields_device in the search's place: d_out [npairs][1][height][width]."""
        self._ck(self.L.gpc_hip_aggregate_batch_device(self.h, C.c_void_p(d_rawL), C.c_void_p(d_rawR), int(width), int(height),
                                                       int(npairs), C.byref(settings), int(refine_radius), C.byref(fill),
                                                       C.byref(aggregate), C.byref(prm), C.c_void_p(d_out), C.c_void_p(d_state or 0),
                                                       C.c_void_p(d_label or 0), C.c_void_p(d_stats or 0), C.c_void_p(d_fwd or 0),
                                                       C.c_void_p(d_level or 0), C.c_void_p(d_counts or 0), C.c_void_p(d_ncand or 0),
                                                       C.c_void_p(d_cost or 0)))

    def aggregate_sequence_device(self, d_frames, width, height, nframes, settings, fill, aggregate, prm, d_out, d_state=0, d_label=0,
                                  d_stats=0, d_fwd=0, d_level=0, refine_radius=0, d_counts=0, d_ncand=0, d_cost=0):
        """search_sequence_device with aggregate_fields_device in the search's place: d_out [nframes-1][2][height][width]."""
        self._ck(self.L.gpc_hip_aggregate_sequence_device(self.h, C.c_void_p(d_frames), int(width), int(height), int(nframes),
                                                          C.byref(settings), int(refine_radius), C.byref(fill), C.byref(aggregate),
                                                          C.byref(prm), C.c_void_p(d_out), C.c_void_p(d_state or 0),
                                                          C.c_void_p(d_label or 0), C.c_void_p(d_stats or 0), C.c_void_p(d_fwd or 0),
                                                          C.c_void_p(d_level or 0), C.c_void_p(d_counts or 0), C.c_void_p(d_ncand or 0),
                                                          C.c_void_p(d_cost or 0)))

    def aggregate_fields(self, field, imgL, imgR, prm=None, want_cost=True, want_choice=True, want_stats=True, want_agg=True):
        """A host field [P, C, height, width] int32 and images [P, height, width] uint8 -> (out [P, C, height, width] int32, cost
        [P, height, width] uint16, choice [P, height, width] uint8, stats [P, 4] int32, agg [P, height, width] uint32; None where
        not wanted)."""
        field = np.ascontiguousarray(field, np.int32)
        imgL, imgR = np.ascontiguousarray(imgL, np.uint8), np.ascontiguousarray(imgR, np.uint8)
        if field.ndim != 4 or field.shape[0] < 1:
            raise ValueError("field: [P, C, height, width] int32")
        P, Cn, H, W = field.shape
        if imgL.shape != (P, H, W) or imgR.shape != (P, H, W):
            raise ValueError("imgL, imgR: [P, height, width] uint8")
        prm = prm if prm is not None else Aggregate()
        out = np.empty(field.shape, np.int32)
        cost = np.empty((P, H, W), np.uint16) if want_cost else None
        choice = np.empty((P, H, W), np.uint8) if want_choice else None
        stats = np.empty((P, 4), np.int32) if want_stats else None
        agg = np.empty((P, H, W), np.uint32) if want_agg else None
        self._ck(self.L.gpc_hip_aggregate_fields(self.h, _ptr(field), _ptr(imgL), _ptr(imgR), Cn, W, H, P, C.byref(prm), _ptr(out),
                                                 _ptr(cost), _ptr(choice), _ptr(stats), _ptr(agg)))
        return out, cost, choice, stats, agg

    # ---- complete cleaned fields (gpc_hip_inpaint_*): holes take the guided weighted mean of the valued pixels around them
    def inpaint_fields_device(self, d_field, d_guide, channels, width, height, npairs, prm, d_out, d_pass=0, d_stats=0):
        """A field [npairs][channels][height][width] int32 and a guide [npairs][height][width] uint8 already in HBM -> d_out of
        the field's shape (it may be d_field itself), d_pass [npairs][height][width] uint8, d_stats [npairs][2] int32 (both
        optional); asynchronous, no forest needed.  Pointers are integers."""
        self._ck(self.L.gpc_hip_inpaint_fields_device(self.h, C.c_void_p(d_field), C.c_void_p(d_guide), int(channels), int(width),
                                                      int(height), int(npairs), C.byref(prm), C.c_void_p(d_out), C.c_void_p(d_pass or 0),
                                                      C.c_void_p(d_stats or 0)))

    def inpaint_batch_device(self, d_rawL, d_rawR, width, height, npairs, settings, fill, prm, inpaint, d_out, d_pass=0, d_fill_stats=0,
                             d_cleaned=0, d_state=0, d_label=0, d_stats=0, d_fwd=0, d_level=0, refine_radius=0, d_counts=0, d_ncand=0):
        """clean_batch_device (its field goes to d_cleaned, optional), then inpaint_fields_device guided by the left images:
        d_out [npairs][1][height][width]."""
        self._ck(self.L.gpc_hip_inpaint_batch_device(self.h, C.c_void_p(d_rawL), C.c_void_p(d_rawR), int(width), int(height), int(npairs),
                                                     C.byref(settings), int(refine_radius), C.byref(fill), C.byref(prm), C.byref(inpaint),
                                                     C.c_void_p(d_out), C.c_void_p(d_pass or 0), C.c_void_p(d_fill_stats or 0),
                                                     C.c_void_p(d_cleaned or 0), C.c_void_p(d_state or 0), C.c_void_p(d_label or 0),
                                                     C.c_void_p(d_stats or 0), C.c_void_p(d_fwd or 0), C.c_void_p(d_level or 0),
                                                     C.c_void_p(d_counts or 0), C.c_void_p(d_ncand or 0)))

    def inpaint_sequence_device(self, d_frames, width, height, nframes, settings, fill, prm, inpaint, d_out, d_pass=0, d_fill_stats=0,
                                d_cleaned=0, d_state=0, d_label=0, d_stats=0, d_fwd=0, d_level=0, refine_radius=0, d_counts=0,
                                d_ncand=0):
        """clean_sequence_device, then inpaint_fields_device guided by frame t: d_out [nframes-1][2][height][width]."""
        self._ck(self.L.gpc_hip_inpaint_sequence_device(self.h, C.c_void_p(d_frames), int(width), int(height), int(nframes),
                                                        C.byref(settings), int(refine_radius), C.byref(fill), C.byref(prm),
                                                        C.byref(inpaint), C.c_void_p(d_out), C.c_void_p(d_pass or 0),
                                                        C.c_void_p(d_fill_stats or 0), C.c_void_p(d_cleaned or 0),
                                                        C.c_void_p(d_state or 0), C.c_void_p(d_label or 0), C.c_void_p(d_stats or 0),
                                                        C.c_void_p(d_fwd or 0), C.c_void_p(d_level or 0), C.c_void_p(d_counts or 0),
                                                        C.c_void_p(d_ncand or 0)))

    def inpaint_fields(self, field, guide, prm=None, want_pass=True, want_stats=True):
        """A host field [P, C, height, width] int32 and guide [P, height, width] uint8 -> (out [P, C, height, width] int32, pass
        [P, height, width] uint8, stats [P, 2] int32; None where not wanted)."""
        field = np.ascontiguousarray(field, np.int32)
        guide = np.ascontiguousarray(guide, np.uint8)
        if field.ndim != 4 or field.shape[0] < 1:
            raise ValueError("field: [P, C, height, width] int32")
        P, Cn, H, W = field.shape
        if guide.shape != (P, H, W):
            raise ValueError("guide: [P, height, width] uint8")
        prm = prm if prm is not None else Inpaint()
        out = np.empty(field.shape, np.int32)
        pas = np.empty((P, H, W), np.uint8) if want_pass else None
        stats = np.empty((P, 2), np.int32) if want_stats else None
        self._ck(self.L.gpc_hip_inpaint_fields(self.h, _ptr(field), _ptr(guide), Cn, W, H, P, C.byref(prm), _ptr(out), _ptr(pas),
                                               _ptr(stats)))
        return out, pas, stats

    # ---- stereo sequences (gpc_hip_quads_*): circular matches closed into quads on the device
    def quads_records_device(self, d_sup, cap_s, d_nsup, d_flowL, d_flowR, cap_f, d_nflowL, d_nflowR, width, height, nframes, tol,
                             d_quads, quad_cap, d_nquads):
        """Device pointers: d_sup [N][cap_s] of SUPPORT_DTYPE, d_nsup [N], d_flowL / d_flowR [N-1][cap_f] of CORR_DTYPE, their
        counts [N-1], d_quads [N-1][quad_cap] of QUAD_DTYPE, d_nquads [N-1] int32; asynchronous, no forest needed."""
        self._ck(self.L.gpc_hip_quads_records_device(self.h, d_sup, int(cap_s), d_nsup, d_flowL, d_flowR, int(cap_f), d_nflowL,
                                                     d_nflowR, int(width), int(height), int(nframes), int(tol), d_quads or 0,
                                                     int(quad_cap), d_nquads))

    def match_stereo_sequence_device(self, d_left, d_right, width, height, nframes, stereo_settings, flow_settings, d_sup, cap_s,
                                     d_nsup, d_flowL, d_flowR, cap_f, d_nflowL, d_nflowR, d_ncand=0):
        """The supports of (L_t, R_t) and the correspondences of (L_t, L_t+1) and (R_t, R_t+1) from one hashing of the 2 N
        images (gpc_hip_match_stereo_sequence_device); d_ncand [2][N] optional."""
        self._ck(self.L.gpc_hip_match_stereo_sequence_device(self.h, d_left, d_right, int(width), int(height), int(nframes),
                                                             C.byref(stereo_settings), C.byref(flow_settings), d_sup, int(cap_s),
                                                             d_nsup, d_flowL, d_flowR, int(cap_f), d_nflowL, d_nflowR, d_ncand or 0))

    def quads_sequence_device(self, d_left, d_right, width, height, nframes, stereo_settings, flow_settings, tol, d_sup, cap_s,
                              d_nsup, d_flowL, d_flowR, cap_f, d_nflowL, d_nflowR, d_ncand, d_quads, quad_cap, d_nquads):
        """match_stereo_sequence_device, then the closing over what it wrote (gpc_hip_quads_sequence_device)."""
        self._ck(self.L.gpc_hip_quads_sequence_device(self.h, d_left, d_right, int(width), int(height), int(nframes),
                                                      C.byref(stereo_settings), C.byref(flow_settings), int(tol), d_sup, int(cap_s),
                                                      d_nsup, d_flowL, d_flowR, int(cap_f), d_nflowL, d_nflowR, d_ncand or 0,
                                                      d_quads or 0, int(quad_cap), d_nquads))

    def quads_records(self, sup, nsup, flowL, nflowL, flowR, nflowR, width, height, tol=1, quad_cap=None, quads_out=None):
        """Host supports [N, cap_s] of SUPPORT_DTYPE with counts [N], correspondences flowL / flowR [N-1, cap_f] of CORR_DTYPE
        with counts [N-1] -> (quads [N-1, quad_cap] of QUAD_DTYPE, nquads [N-1], status).  Quads beyond min(nquads[t],
        quad_cap) are left as they were (zero in an array made here).  quad_cap None: cap_s, which always suffices."""
        sup, flowL, flowR = (a if a.flags.c_contiguous else np.ascontiguousarray(a) for a in map(np.asarray, (sup, flowL, flowR)))
        if sup.dtype != SUPPORT_DTYPE or sup.ndim != 2 or sup.shape[0] < 2 or sup.shape[1] < 1:
            raise ValueError("sup: [N, cap_s] of SUPPORT_DTYPE, N >= 2")
        N, cap_s = sup.shape
        if flowL.dtype != CORR_DTYPE or flowR.dtype != CORR_DTYPE or flowL.shape != flowR.shape or flowL.ndim != 2 or \
                flowL.shape[0] != N - 1 or flowL.shape[1] < 1:
            raise ValueError("flowL, flowR: [N - 1, cap_f] of CORR_DTYPE")
        cap_f = flowL.shape[1]
        nsup, nflowL, nflowR = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (nsup, nflowL, nflowR))
        if len(nsup) != N or len(nflowL) != N - 1 or len(nflowR) != N - 1:
            raise ValueError("counts: one per frame / step")
        quad_cap = cap_s if quad_cap is None else int(quad_cap)
        quads = quads_out if quads_out is not None else np.zeros((N - 1, max(quad_cap, 1)), QUAD_DTYPE)
        nquads = np.zeros(N - 1, np.int32)
        st = self.L.gpc_hip_quads_records(self.h, _ptr(sup), cap_s, _ptr(nsup), _ptr(flowL), _ptr(flowR), cap_f, _ptr(nflowL),
                                          _ptr(nflowR), int(width), int(height), N, int(tol), _ptr(quads), quad_cap, _ptr(nquads))
        self._ck(st, allow=(E_CAPACITY,))
        return quads, nquads, st

    def quads_sequence(self, left, right, stereo_settings, flow_settings, tol=1, cap_s=None, cap_f=None, quad_cap=None, alloc=None):
        """left, right [N, H, W] uint8 -> dict(sup, nsup, flowL, nflowL, flowR, nflowR, ncand [2, N], quads, nquads, status):
        the three record sets of the stereo sequence and its quads (gpc_hip_quads_sequence).  alloc(shape, dtype): where
        the output arrays come from (np.zeros; Context.pinned_empty for page-locked ones)."""
        left, right = _host_frames(left), _host_frames(right)
        if left.shape != right.shape:
            raise ValueError("left and right: the same [N, H, W]")
        N, H, W = left.shape
        inner = max((W - 26) * (H - 26), 1)
        cap_s = inner if cap_s is None else int(cap_s)
        cap_f = inner if cap_f is None else int(cap_f)
        quad_cap = cap_s if quad_cap is None else int(quad_cap)
        alloc = alloc or (lambda shape, dtype: np.zeros(shape, dtype))
        o = dict(sup=alloc((N, cap_s), SUPPORT_DTYPE), nsup=alloc((N,), np.int32), flowL=alloc((N - 1, cap_f), CORR_DTYPE),
                 nflowL=alloc((N - 1,), np.int32), flowR=alloc((N - 1, cap_f), CORR_DTYPE), nflowR=alloc((N - 1,), np.int32),
                 ncand=alloc((2, N), np.int32), quads=alloc((N - 1, max(quad_cap, 1)), QUAD_DTYPE), nquads=alloc((N - 1,), np.int32))
        st = self.L.gpc_hip_quads_sequence(self.h, _ptr(left), _ptr(right), W, H, N, C.byref(stereo_settings), C.byref(flow_settings),
                                           int(tol), _ptr(o["sup"]), cap_s, _ptr(o["nsup"]), _ptr(o["flowL"]), _ptr(o["flowR"]), cap_f,
                                           _ptr(o["nflowL"]), _ptr(o["nflowR"]), _ptr(o["ncand"]), _ptr(o["quads"]), quad_cap,
                                           _ptr(o["nquads"]))
        self._ck(st, allow=(E_CAPACITY,))
        o["status"] = st
        return o

    # ---- fern training: the scoring loop
    def train_set(self, triplets):
        """Uploads (n, 3, 729) uint8 patch triplets (ref, pos, neg); returns a TrainSet."""
        return TrainSet(self, triplets)

    def extract_triplets(self, rawL, rawR, pts, frame_first, order=None):
        """Feature::extractAllTriplets for a batch of frame pairs (gpc_hip_extract_triplets), straight into a TrainSet.
        rawL, rawR: (nframes, H, W) uint8 numpy arrays or CPU tensors (host entry point), or contiguous torch.uint8 tensors
        on this context's GPU (the _device entry point; a tensor on another device is refused); pts: POINTS_DTYPE records
        (or an (n, 6) int array) of all frames back to back; frame_first: nframes + 1 ascending offsets into pts, the last
        one len(pts); order: None or a permutation of the kept triplets.  Returns None when no triplet is kept.
        Anything else raises ValueError before the library is called: the C entry points trust these lengths."""
        dev = _device_frames(rawL, rawR, self.device)
        if dev:
            if rawL.shape != rawR.shape or rawL.dim() != 3:
                raise ValueError("rawL / rawR: (nframes, H, W) tensors of one shape")
            nframes, H, W = rawL.shape
            pL, pR = C.c_void_p(rawL.data_ptr()), C.c_void_p(rawR.data_ptr())
            fn = self.L.gpc_hip_extract_triplets_device
        else:
            rawL, rawR = _host_frames(rawL), _host_frames(rawR)
            if rawL.ndim != 3 or rawL.shape != rawR.shape:
                raise ValueError("rawL / rawR: (nframes, H, W) arrays of one shape")
            nframes, H, W = rawL.shape
            pL, pR = _ptr(rawL), _ptr(rawR)
            fn = self.L.gpc_hip_extract_triplets
        p = np.asarray(pts)
        if p.dtype != POINTS_DTYPE:
            p = np.ascontiguousarray(p, np.int32)
            if p.size % 6:
                raise ValueError("pts: six coordinates per triplet")
            p = p.reshape(-1, 6).view(POINTS_DTYPE).reshape(-1)
        p = np.ascontiguousarray(p).reshape(-1)
        ff = np.ascontiguousarray(frame_first, np.int32).reshape(-1)
        if len(ff) != nframes + 1 or ff[0] != 0 or (np.diff(ff) < 0).any() or ff[-1] != len(p):
            raise ValueError("frame_first: nframes + 1 ascending offsets from 0 to len(pts)")
        o = None
        if order is not None:
            o = np.ascontiguousarray(order, np.int32).reshape(-1)
            n_kept = kept_count(p, W, H)
            if len(o) != n_kept:
                raise ValueError("order: %d entries for %d kept triplets" % (len(o), n_kept))
        h = C.c_void_p()
        n = C.c_int()
        self._ck(fn(self.h, pL, pR, int(W), int(H), int(nframes), _ptr(p) if len(p) else None, _ptr(ff), _ptr(o),
                    C.byref(h), C.byref(n)))
        if n.value == 0:
            return None
        return TrainSet(self, handle=h, n=n.value)

    # ---- measurement
    def enable_kernel_timing(self, on=True, only=None):
        """HIP-event bracketing of kernel launches; `only` = iterable of kernel names to restrict it to."""
        mask = 0xFFFFFFFF
        if only is not None:
            names = [self.L.gpc_hip_kernel_name(i).decode() for i in range(self.L.gpc_hip_kernel_slots())]
            mask = 0
            for n in only:
                if names.index(n) < 32:     # (the slots behind the mask are always bracketed)
                    mask |= 1 << names.index(n)
        self._ck(self.L.gpc_hip_set_kernel_timing_mask(self.h, mask))
        self._ck(self.L.gpc_hip_enable_kernel_timing(self.h, int(on)))

    def reset_kernel_timing(self):
        self._ck(self.L.gpc_hip_reset_kernel_timing(self.h))

    def kernel_launch_names(self):
        """{timing slot name: rocprofv3 name of the instantiation last launched there}"""
        return {self.L.gpc_hip_kernel_name(i).decode(): self.L.gpc_hip_kernel_launch_name(self.h, i).decode()
                for i in range(self.L.gpc_hip_kernel_slots())}

    def kernel_times(self):
        """{kernel name: (total ms, launches)} since the last reset."""
        out = {}
        for i in range(self.L.gpc_hip_kernel_slots()):
            ms, n = C.c_float(), C.c_int()
            self._ck(self.L.gpc_hip_kernel_time(self.h, i, C.byref(ms), C.byref(n)))
            out[self.L.gpc_hip_kernel_name(i).decode()] = (ms.value, n.value)
        return out


class TrackStream:
    """One gpc_hip_track_stream of a Context: what the offline track calls return for the frames (or records) pushed so
    far, delivered push by push.  The device forms take raw device pointers and only queue work (the device-wide matchers
    wait once inside the call); push() takes host frames and is synchronous."""

    def __init__(self, ctx, width, height, settings, cap_per_pair, track_cap):
        self.ctx = ctx
        self.h = None
        self.width, self.height, self.cap, self.track_cap = int(width), int(height), int(cap_per_pair), int(track_cap)
        h = C.c_void_p()
        ctx._ck(ctx.L.gpc_hip_track_stream_create(ctx.h, self.width, self.height, C.byref(settings) if settings is not None else None,
                                                  self.cap, self.track_cap, C.byref(h)))
        self.h = h

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.L.gpc_hip_track_stream_destroy(self.ctx.h, self.h)
        self.h = None

    def reset(self):
        self.ctx._ck(self.ctx.L.gpc_hip_track_stream_reset(self.ctx.h, self.h))

    def push_device(self, d_frames, nframes, d_corr, d_counts, d_ncand, d_prev, d_track_id):
        """nframes frames in HBM -> the number of pairs produced; outputs [k][cap] (d_ncand [nframes], optional)"""
        k = C.c_int()
        self.ctx._ck(self.ctx.L.gpc_hip_track_stream_push_device(self.ctx.h, self.h, C.c_void_p(d_frames), int(nframes),
                                                                 C.c_void_p(d_corr), C.c_void_p(d_counts), C.c_void_p(d_ncand or 0),
                                                                 C.c_void_p(d_prev), C.c_void_p(d_track_id), C.byref(k)))
        return k.value

    def push_records_device(self, d_corr, d_counts, npairs, d_prev, d_track_id):
        self.ctx._ck(self.ctx.L.gpc_hip_track_stream_push_records_device(self.ctx.h, self.h, C.c_void_p(d_corr), C.c_void_p(d_counts),
                                                                         int(npairs), C.c_void_p(d_prev), C.c_void_p(d_track_id)))

    def push(self, frames, fill=-1, alloc=None):
        """Host frames [n, H, W] (or one frame [H, W]) -> (records [k, cap] of CORR_DTYPE, counts [k], ncand [n], prev [k, cap],
        track_id [k, cap], n_tracks so far, status); entries of prev / track_id beyond a pair's count hold `fill`.
        alloc(shape, dtype): where the outputs are made (np.empty; Context.pinned_empty for page-locked ones)."""
        frames = np.asarray(frames)
        if frames.ndim == 2:
            frames = frames[None]
        frames = _host_frames(frames)
        n, H, W = frames.shape
        if (W, H) != (self.width, self.height):
            raise ValueError("frames must be %d x %d" % (self.width, self.height))
        alloc = alloc or np.empty
        rows = max(n, 1)
        out = alloc((rows, self.cap), CORR_DTYPE)
        counts = alloc((rows,), np.int32)
        ncand = alloc((rows,), np.int32)
        prev = alloc((rows, self.cap), np.int32)
        tid = alloc((rows, self.cap), np.int32)
        prev[...] = fill
        tid[...] = fill
        k, total = C.c_int(), C.c_int32()
        st = self.ctx.L.gpc_hip_track_stream_push(self.ctx.h, self.h, _ptr(frames), n, _ptr(out), _ptr(counts), _ptr(ncand),
                                                  _ptr(prev), _ptr(tid), C.byref(k), C.byref(total))
        self.ctx._ck(st, allow=(E_CAPACITY,))
        k = k.value
        return out[:k], counts[:k], ncand[:n], prev[:k], tid[:k], total.value, st

    def state(self):
        """(frames seen, pairs seen, tracks so far); waits for the context's stream"""
        f, p, n = C.c_int(), C.c_int(), C.c_int32()
        self.ctx._ck(self.ctx.L.gpc_hip_track_stream_state(self.ctx.h, self.h, C.byref(f), C.byref(p), C.byref(n)))
        return f.value, p.value, n.value

    def table(self):
        """(device pointer of the table [track_cap] of TRACK_DTYPE, device pointer of the int32 total)"""
        t, n = C.c_void_p(), C.c_void_p()
        self.ctx._ck(self.ctx.L.gpc_hip_track_stream_table(self.h, C.byref(t), C.byref(n)))
        return t.value, n.value

    def read_tracks(self, first=0, n=None, fill=-1):
        """(rows [first, first + n) that exist as a TRACK_DTYPE array, tracks so far); n None: up to the table's end"""
        n = self.track_cap - first if n is None else int(n)
        rows = np.full((max(n, 1), 4), fill, np.int32)
        total = C.c_int32()
        self.ctx._ck(self.ctx.L.gpc_hip_track_stream_read_tracks(self.ctx.h, self.h, int(first), n, _ptr(rows), C.byref(total)))
        have = max(0, min(first + n, total.value) - first)
        return rows[:have].view(TRACK_DTYPE).reshape(-1), total.value


class TrainSet:
    """Device-resident training triplets of one Context (gpc_hip_train_set): Fern::evalSplit,
    Fern::markSplitSamples and Fern::train (with caller-supplied hyperplane samples) on the GPU."""

    def __init__(self, ctx, triplets=None, handle=None, n=0):
        self.ctx = ctx
        if handle is not None:  # a set the library made (Context.extract_triplets)
            self.n = int(n)
            self.h = handle
            return
        t = np.ascontiguousarray(triplets, np.uint8)
        if t.ndim != 3 or t.shape[1:] != (3, PATCH_BYTES):
            raise ValueError("triplets must have shape (n, 3, 729)")
        self.n = len(t)
        h = C.c_void_p()
        ctx._ck(ctx.L.gpc_hip_train_set_create(ctx.h, _ptr(t), self.n, C.byref(h)))
        self.h = h

    def read(self, first=0, n=None):
        """Triplets [first, first + n) as an (n, 3, 729) uint8 array (gpc_hip_train_set_read)."""
        n = self.n - first if n is None else int(n)
        out = np.empty((max(n, 0), 3, PATCH_BYTES), np.uint8)
        self.ctx._ck(self.ctx.L.gpc_hip_train_set_read(self.ctx.h, self.h, int(first), n, _ptr(out)))
        return out

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.L.gpc_hip_train_set_destroy(self.ctx.h, self.h)
        self.h = None

    def marks(self, new=None):
        """Reads (and optionally first replaces) the split marks: bit 0 pos.split, bit 1 neg.split."""
        out = np.empty(self.n, np.uint8)
        src = None if new is None else np.ascontiguousarray(new, np.uint8)
        self.ctx._ck(self.ctx.L.gpc_hip_train_set_marks(self.ctx.h, self.h, _ptr(src), _ptr(out)))
        return out

    def eval_split(self, params, score_until_level, w1):
        p = np.ascontiguousarray(params, SPLIT_DTYPE)
        st = np.zeros(1, STATS_DTYPE)
        self.ctx._ck(self.ctx.L.gpc_hip_train_eval_split(self.ctx.h, self.h, _ptr(p), int(score_until_level),
                                                         C.c_double(w1), _ptr(st)))
        return st[0]

    def mark_split_samples(self, params, num_params):
        p = np.ascontiguousarray(params, SPLIT_DTYPE)
        self.ctx._ck(self.ctx.L.gpc_hip_train_mark_split_samples(self.ctx.h, self.h, _ptr(p), int(num_params)))

    def train_fern(self, max_depth, cand, num_resamples, taulo, tauhi, only_score_non_split, w1):
        """cand[level * num_resamples + k] = k-th hyperplane sample of `level`.  Returns (params, stats)."""
        c = np.ascontiguousarray(cand, SPLIT_DTYPE)
        if len(c) < max_depth * num_resamples:
            raise ValueError("need max_depth * num_resamples hyperplane samples")
        fp = np.zeros(max_depth, SPLIT_DTYPE)
        st = np.zeros(max_depth, STATS_DTYPE)
        self.ctx._ck(self.ctx.L.gpc_hip_train_fern(self.ctx.h, self.h, int(max_depth), _ptr(c), int(num_resamples),
                                                   int(taulo), int(tauhi), int(bool(only_score_non_split)),
                                                   C.c_double(w1), _ptr(fp), _ptr(st)))
        return fp, st

    def train_forest(self, nferns, max_depth, cand, num_resamples, taulo, tauhi, only_score_non_split, w1, draws=None):
        """Every fern of a forest over this one resident set (gpc_hip_train_forest).  cand[f, level, k] = fern f's k-th
        hyperplane sample of `level`; draws[f, d] = index into the set of fern f's d-th bootstrap draw (None: every fern
        trains on the whole set).  Returns (params[nferns, max_depth], stats[nferns, max_depth]); the set's marks stay."""
        c = np.ascontiguousarray(cand, SPLIT_DTYPE).reshape(-1)
        if len(c) < nferns * max_depth * num_resamples:
            raise ValueError("need nferns * max_depth * num_resamples hyperplane samples")
        d, per_fern = None, 0
        if draws is not None:
            d = np.ascontiguousarray(draws, np.int32)
            if d.ndim != 2 or d.shape[0] != nferns:
                raise ValueError("draws must have shape (nferns, draws_per_fern)")
            per_fern = d.shape[1]
        shape = (max(nferns, 0), max(max_depth, 0))
        fp = np.zeros(shape, SPLIT_DTYPE)
        st = np.zeros(shape, STATS_DTYPE)
        self.ctx._ck(self.ctx.L.gpc_hip_train_forest(self.ctx.h, self.h, int(nferns), int(max_depth), _ptr(c),
                                                     int(num_resamples), int(taulo), int(tauhi),
                                                     int(bool(only_score_non_split)), C.c_double(w1), _ptr(d), per_fern,
                                                     _ptr(fp), _ptr(st)))
        return fp, st

    def begin_fern(self, reset_marks):
        self.ctx._ck(self.ctx.L.gpc_hip_train_begin_fern(self.ctx.h, self.h, int(bool(reset_marks))))

    def eval_level(self, cand, taulo, tauhi):
        """tp, fp of every (candidate, tau) of the current level and the number of samples that count."""
        c = np.ascontiguousarray(cand, SPLIT_DTYPE)
        ntau = tauhi - taulo
        tp = np.zeros((len(c), max(ntau, 0)), np.int32)
        fp = np.zeros_like(tp)
        tot = np.zeros(1, np.int32)
        self.ctx._ck(self.ctx.L.gpc_hip_train_eval_level(self.ctx.h, self.h, _ptr(c), len(c), int(taulo), int(tauhi),
                                                         _ptr(tp), _ptr(fp), _ptr(tot)))
        return tp, fp, int(tot[0])

    def commit_level(self, best, mark_split):
        b = np.ascontiguousarray(best, SPLIT_DTYPE).reshape(1)
        self.ctx._ck(self.ctx.L.gpc_hip_train_commit_level(self.ctx.h, self.h, _ptr(b), int(bool(mark_split))))
