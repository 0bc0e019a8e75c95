"""ctypes binding of libopenpose_hip.so (C ABI: include/openpose_hip.h).

There is no CPU fallback: if the HIP library is missing or cannot load, every entry point
raises.  Status codes map to the exceptions the reference would raise (IndexError for the
grouping overflow at pose_detector.py:197) or to RuntimeError/ValueError.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# OP_LIB_VARIANT=<name> loads libopenpose_hip.<name>.so instead (kernel tuning experiments only)
LIB_PATH = os.path.join(_HERE, "libopenpose_hip%s.so" % (
    "." + os.environ["OP_LIB_VARIANT"] if os.environ.get("OP_LIB_VARIANT") else ""))

OP_OK, OP_ERR_INVALID, OP_ERR_HIP, OP_ERR_CAPACITY, OP_ERR_INDEX, OP_ERR_STATE, OP_ERR_TIMEOUT = range(7)
OP_COMM_ID_BYTES = 128
N_JOINTS, N_LIMBS, N_PAF, N_HEAT, N_LAYERS = 18, 19, 38, 19, 92

# Every symbol include/openpose_hip.h declares (checked by tests/test_abi.py).
EXPORTED = (
    "op_last_error", "op_build_info", "op_default_params", "op_default_limits", "op_layer_info", "op_create", "op_destroy",
    "op_set_weights", "op_detect", "op_preprocess", "op_forward", "op_forward_stages", "op_forward_probe",
    "op_forward_probe_info", "op_resize_images", "op_compute_peaks",
    "op_compute_connections", "op_grouping", "op_postprocess", "op_stage_frames", "op_stage_maps",
    "op_use_staged_maps", "op_run_staged", "op_run_staged_graph", "op_graph_info", "op_synchronize", "op_fetch_result",
    "op_last_timing", "op_forward_flops", "op_profile_enable", "op_profile_read", "op_profile_reset",
    "op_set_precision", "op_get_precision", "op_fetch_results", "op_fetch_maps", "op_upload_frames", "op_upload_wait", "op_conv_census", "op_host_alloc", "op_host_free",
    "op_pack_results", "op_comm_unique_id", "op_comm_create", "op_comm_destroy", "op_comm_gather_results",
    "op_comm_wait", "op_comm_overflow", "op_comm_overflow_result", "op_detect_precise", "op_resize_cubic",
    "op_set_conv_algo", "op_set_stage_layout", "op_set_batch_invariant", "op_set_peak_mode", "op_profile_classes", "op_run_staged_precise",
    "op_cpm_layer_count", "op_cpm_layer_info", "op_cpm_create", "op_cpm_destroy", "op_cpm_set_weights",
    "op_cpm_forward", "op_cpm_peaks", "op_cpm_detect", "op_cpm_detect_batch", "op_cpm_set_batch_invariant",
    "op_cpm_probe_info", "op_cpm_forward_probe",
    "op_cpm_detect_rois", "op_cpm_set_roi_group_bytes", "op_cpm_roi_stats",
    "op_train_create", "op_train_destroy", "op_train_set_weights", "op_train_get_weights", "op_train_set_hyper",
    "op_train_enable_layer", "op_train_set_grad_scale", "op_train_step",
    "op_make_labels", "op_train_step_poses", "op_train_last_label_ms",
    "op_train_eval", "op_train_eval_poses", "op_train_get_state", "op_train_set_state",
    "op_train_buffer_info", "op_train_read_buffer",
    "op_augment", "op_augment_last_ms", "op_augment_last_paths", "op_augment_tables",
    "op_ignore_masks", "op_ignore_masks_last_ms",
    "op_annotation_views", "op_annotation_views_last_ms",
    "op_draw", "op_draw_staged", "op_staged_info", "op_draw_last_ms",
    "op_overlay", "op_overlay_staged", "op_overlay_last_ms",
    "op_cpm_detect_rois_staged", "op_cpm_set_roi_batch",
    "op_body_rois", "op_body_rois_staged", "op_body_last_ms",
    "op_keypoint_match", "op_keypoint_match_staged", "op_keypoint_last_ms",
    "op_jpeg_probe", "op_jpeg_coefficients", "op_jpeg_block_in_range", "op_jpeg_decode", "op_jpeg_stage",
    "op_jpeg_set_threads", "op_jpeg_last_ms",
    "op_haar_create", "op_haar_destroy", "op_haar_detect", "op_haar_candidates", "op_haar_detect_staged",
    "op_haar_probe", "op_haar_last_ms",
)
ARCH = {"facenet": 1, "handnet": 2}
CPM_PROBE_HI = 256  # OP_CPM_PROBE_HI
MAX_SCALES = 8
PRECISION = {"fp32": 0, "bf16x3": 1}
PEAK_BRANCH = {"cpu": 0, "gpu": 1}  # OP_PEAKS_CPU_BRANCH / OP_PEAKS_GPU_BRANCH


class OpParams(ctypes.Structure):
    _fields_ = [
        ("inference_img_size", ctypes.c_int32), ("heatmap_size", ctypes.c_int32),
        ("gaussian_sigma", ctypes.c_double), ("n_integ_points", ctypes.c_int32),
        ("n_integ_points_thresh", ctypes.c_int32), ("heatmap_peak_thresh", ctypes.c_double),
        ("inner_product_thresh", ctypes.c_double), ("limb_length_ratio", ctypes.c_double),
        ("length_penalty_value", ctypes.c_double), ("n_subset_limbs_thresh", ctypes.c_int32),
        ("subset_score_thresh", ctypes.c_double), ("limbs_point", (ctypes.c_int32 * 2) * N_LIMBS),
        ("downscale", ctypes.c_int32), ("n_scales", ctypes.c_int32),
        ("inference_scales", ctypes.c_double * MAX_SCALES),
    ]


class OpLimits(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "max_batch", "max_net_h", "max_net_w", "max_map_h", "max_map_w", "max_peaks_per_joint",
        "max_frame_h", "max_frame_w")]


class OpFrameResult(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "status", "n_peaks", "n_persons", "map_w", "map_h", "net_w", "net_h")]


class OpDrawPrim(ctypes.Structure):
    """op_draw_prim (include/openpose_hip.h): one primitive of a display list (render.py)."""
    _fields_ = [("kind", ctypes.c_int32), ("radius", ctypes.c_int32),
                ("x0", ctypes.c_double), ("y0", ctypes.c_double), ("x1", ctypes.c_double), ("y1", ctypes.c_double),
                ("thickness", ctypes.c_double),
                ("wa", ctypes.c_double), ("wb", ctypes.c_double), ("gamma", ctypes.c_double),
                ("bgr", ctypes.c_uint8 * 3), ("pad", ctypes.c_uint8 * 5)]


OP_DRAW_LINE, OP_DRAW_DISC, OP_DRAW_BLEND = range(3)


class OpJpegInfo(ctypes.Structure):
    """op_jpeg_info (include/openpose_hip.h): what a file's headers say (op_jpeg_probe)."""
    _fields_ = [("status", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("components", ctypes.c_int32),
                ("hs", ctypes.c_int32), ("vs", ctypes.c_int32), ("blocks_w", ctypes.c_int32 * 3),
                ("blocks_h", ctypes.c_int32 * 3), ("n_blocks", ctypes.c_int64)]


class OpHaarParams(ctypes.Structure):
    """op_haar_params (include/openpose_hip.h): detectMultiScale's arguments."""
    _fields_ = [("scale_factor", ctypes.c_double), ("min_neighbors", ctypes.c_int32), ("min_w", ctypes.c_int32),
                ("min_h", ctypes.c_int32), ("has_max", ctypes.c_int32), ("max_w", ctypes.c_int32),
                ("max_h", ctypes.c_int32), ("max_candidates", ctypes.c_int32)]


HAAR_MAX_SCALES, HAAR_TIMES = 64, ("total", "grey", "pyramid", "integrals", "cascade")

_lib = None


def lib():
    """Load the HIP library (fails loudly: there is no other implementation of this path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libopenpose_hip.so is not built (%s); run __graft_entry__.build() or "
                           "make -C chainer_realtime_multi-person_pose_estimation_amd/csrc" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    P, I32, I64, D = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    sig = {
        "op_last_error": ([], ctypes.c_char_p),
        "op_build_info": ([ctypes.c_char_p, I32], ctypes.c_int),
        "op_default_params": ([P], ctypes.c_int),
        "op_default_limits": ([P], ctypes.c_int),
        "op_layer_info": ([ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), P, P, P], ctypes.c_int),
        "op_create": ([P, P, ctypes.c_int, P], ctypes.c_int),
        "op_destroy": ([P], ctypes.c_int),
        "op_set_weights": ([P, P, P], ctypes.c_int),
        "op_detect": ([P, P, I32, I32, I64, P, P, I32, P], ctypes.c_int),
        "op_detect_precise": ([P, P, I32, I32, I64, P, P, I32, P, P, P], ctypes.c_int),
        "op_set_conv_algo": ([P, I32], ctypes.c_int),
        "op_set_stage_layout": ([P, I32], ctypes.c_int),
        "op_set_batch_invariant": ([P, I32], ctypes.c_int),
        "op_set_peak_mode": ([P, I32, I32], ctypes.c_int),
        "op_profile_classes": ([P, I32], ctypes.c_int),
        "op_resize_cubic": ([P, P, I32, I32, I32, I32, P, I32, I32], ctypes.c_int),
        "op_preprocess": ([P, P, I32, I32, I64, I32, I32, P], ctypes.c_int),
        "op_forward": ([P, P, I32, I32, I32, P, P], ctypes.c_int),
        "op_forward_stages": ([P, P, I32, I32, I32, P, P], ctypes.c_int),
        "op_forward_probe": ([P, P, I32, I32, I32, I32, I32, I32, P, I64], ctypes.c_int),
        "op_forward_probe_info": ([I32, ctypes.POINTER(ctypes.c_char_p), P, P], ctypes.c_int),
        "op_resize_images": ([P, P, I32, I32, I32, I32, I32, P], ctypes.c_int),
        "op_compute_peaks": ([P, P, I32, I32, I32, P, I64, P], ctypes.c_int),
        "op_compute_connections": ([P, P, I32, I32, P, I64, D, P, I64, P], ctypes.c_int),
        "op_grouping": ([P, P, P, P, I64, P, I64, P], ctypes.c_int),
        "op_postprocess": ([P, P, P, I32, I32, I32, I32, P, P, I32, P], ctypes.c_int),
        "op_stage_frames": ([P, P, I32, I32, I32], ctypes.c_int),
        "op_stage_maps": ([P, P, I32, I32, I32], ctypes.c_int),
        "op_use_staged_maps": ([P, I32], ctypes.c_int),
        "op_run_staged": ([P], ctypes.c_int),
        "op_run_staged_graph": ([P], ctypes.c_int),
        "op_graph_info": ([P, P, P, P, P, P], ctypes.c_int),
        "op_run_staged_precise": ([P], ctypes.c_int),
        "op_synchronize": ([P], ctypes.c_int),
        "op_fetch_result": ([P, I32, P, P, I32, P], ctypes.c_int),
        "op_last_timing": ([P, P, P, P], ctypes.c_int),
        "op_forward_flops": ([I32, I32], D),
        "op_profile_enable": ([P, I32], ctypes.c_int),
        "op_profile_read": ([P, I32, P, P, P, P], ctypes.c_int),
        "op_profile_reset": ([P], ctypes.c_int),
        "op_set_precision": ([P, I32], ctypes.c_int),
        "op_get_precision": ([P, P], ctypes.c_int),
        "op_fetch_results": ([P, I32, I32, P, P, I32, P], ctypes.c_int),
        "op_cpm_layer_count": ([I32], ctypes.c_int),
        "op_cpm_layer_info": ([I32, I32, ctypes.POINTER(ctypes.c_char_p), P, P, P], ctypes.c_int),
        "op_cpm_create": ([I32, I32, P], ctypes.c_int),
        "op_cpm_destroy": ([P], ctypes.c_int),
        "op_cpm_set_weights": ([P, P, P], ctypes.c_int),
        "op_cpm_forward": ([P, P, I32, I32, I32, P], ctypes.c_int),
        "op_cpm_probe_info": ([I32, I32, ctypes.POINTER(ctypes.c_char_p), P, P], ctypes.c_int),
        "op_cpm_forward_probe": ([P, P, I32, I32, I32, I32, I32, I32, P, I64], ctypes.c_int),
        "op_cpm_peaks": ([P, P, I32, I32, I32, ctypes.c_float, I32, P, P], ctypes.c_int),
        "op_cpm_detect": ([P, P, I32, I32, I64, ctypes.c_float, I32, P, P], ctypes.c_int),
        "op_cpm_detect_batch": ([P, I32, P, P, P, P, ctypes.c_float, P, P, P], ctypes.c_int),
        "op_pack_results": ([P, I32, I32, I32, ctypes.c_int64, I32, P], ctypes.c_int),
        "op_comm_unique_id": ([P], ctypes.c_int),
        "op_comm_create": ([P, I32, I32, P, ctypes.c_double, P], ctypes.c_int),
        "op_comm_destroy": ([P], ctypes.c_int),
        "op_comm_gather_results": ([P, P, I32, I32, I32, ctypes.c_int64, I32], ctypes.c_int),
        "op_comm_wait": ([P, ctypes.c_double, P, P, P], ctypes.c_int),
        "op_comm_overflow": ([P, P, P, P, I32, P], ctypes.c_int),
        "op_comm_overflow_result": ([P, P, I32, P, P, I32, P], ctypes.c_int),
        "op_upload_frames": ([P, P, I32, I32, I32], ctypes.c_int),
        "op_upload_wait": ([P], ctypes.c_int),
        "op_conv_census": ([P, I32, I32], ctypes.c_int),
        "op_host_alloc": ([ctypes.c_size_t, P], ctypes.c_int),
        "op_host_free": ([P], ctypes.c_int),
        "op_fetch_maps": ([P, I32, I32, P, P, P, P], ctypes.c_int),
        "op_cpm_set_batch_invariant": ([P, I32], ctypes.c_int),
        "op_cpm_detect_rois": ([P, I32, P, P, P, P, I32, P, P, P, ctypes.c_float, P, P], ctypes.c_int),
        "op_cpm_set_roi_group_bytes": ([P, I64], ctypes.c_int),
        "op_cpm_roi_stats": ([P, P], ctypes.c_int),
        "op_train_create": ([I32, I32, I32, I32, P], ctypes.c_int),
        "op_train_destroy": ([P], ctypes.c_int),
        "op_train_set_weights": ([P, P, P], ctypes.c_int),
        "op_train_get_weights": ([P, P, P, P, P], ctypes.c_int),
        "op_train_set_hyper": ([P, D, D, D, D], ctypes.c_int),
        "op_train_enable_layer": ([P, I32, I32], ctypes.c_int),
        "op_train_set_grad_scale": ([P, I32, D], ctypes.c_int),
        "op_train_step": ([P, P, P, P, P, P], ctypes.c_int),
        "op_make_labels": ([I32, I32, I32, I32, I32, P, P, P, D, D, P, P, P], ctypes.c_int),
        "op_train_step_poses": ([P, P, P, P, P, D, D, P], ctypes.c_int),
        "op_train_last_label_ms": ([P, P], ctypes.c_int),
        "op_train_eval": ([P, I32, P, P, P, P, P], ctypes.c_int),
        "op_train_eval_poses": ([P, I32, P, P, P, P, D, D, P], ctypes.c_int),
        "op_train_get_state": ([P, P, P, P, P, P], ctypes.c_int),
        "op_train_set_state": ([P, P, P, P, P, P], ctypes.c_int),
        "op_train_buffer_info": ([I32, ctypes.POINTER(ctypes.c_char_p), P, P], ctypes.c_int),
        "op_train_read_buffer": ([P, I32, I32, P, I64], ctypes.c_int),
        "op_augment": ([I32, I32, P, P, P, P, I32, P, P], ctypes.c_int),
        "op_augment_last_ms": ([I32, P], ctypes.c_int),
        "op_augment_last_paths": ([I32, P], ctypes.c_int),
        "op_augment_tables": ([P, P, P, P], ctypes.c_int),
        "op_ignore_masks": ([I32, I32, P, P, P, P, P, P, P, P, P, P, P], ctypes.c_int),
        "op_ignore_masks_last_ms": ([I32, P], ctypes.c_int),
        "op_annotation_views": ([I32, I32, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P], ctypes.c_int),
        "op_annotation_views_last_ms": ([I32, P], ctypes.c_int),
        "op_draw": ([I32, I32, P, P, P, P, P, P], ctypes.c_int),
        "op_draw_staged": ([P, I32, I32, P, P, P], ctypes.c_int),
        "op_staged_info": ([P, P, P, P], ctypes.c_int),
        "op_draw_last_ms": ([I32, P], ctypes.c_int),
        "op_overlay": ([I32, I32, P, P, P, P, P, P, P, P, P, P, P], ctypes.c_int),
        "op_overlay_staged": ([P, I32, I32, I32, P, P], ctypes.c_int),
        "op_overlay_last_ms": ([I32, P], ctypes.c_int),
        "op_cpm_detect_rois_staged": ([P, P, I32, I32, I32, P, P, P, ctypes.c_float, P, P], ctypes.c_int),
        "op_cpm_set_roi_batch": ([P, I32], ctypes.c_int),
        "op_body_rois": ([I32, I32, P, P, P, P], ctypes.c_int),
        "op_body_rois_staged": ([P, I32, I32, I32, P, P, P, P, P], ctypes.c_int),
        "op_body_last_ms": ([I32, P], ctypes.c_int),
        "op_keypoint_match": ([I32, I32] + [P] * 9 + [I32, I32, P, I32, P, P] + [P] * 6, ctypes.c_int),
        "op_keypoint_match_staged": ([P, I32, I32] + [P] * 7 + [I32, I32, P, I32, P, P] + [P] * 9, ctypes.c_int),
        "op_keypoint_last_ms": ([I32, P], ctypes.c_int),
        "op_jpeg_probe": ([P, I64, P], ctypes.c_int),
        "op_jpeg_coefficients": ([P, I64, P, I64, P, P], ctypes.c_int),
        "op_jpeg_block_in_range": ([P, P, P], ctypes.c_int),
        "op_jpeg_decode": ([I32, I32, P, P, P, P], ctypes.c_int),
        "op_jpeg_stage": ([P, I32, P, P, P, I32, I32, P], ctypes.c_int),
        "op_jpeg_set_threads": ([I32], ctypes.c_int),
        "op_jpeg_last_ms": ([I32, P], ctypes.c_int),
        "op_haar_create": ([I32, I32, I32, I32, P, P, I32, P, P, P, P, P, P], ctypes.c_int),
        "op_haar_destroy": ([P], ctypes.c_int),
        "op_haar_detect": ([P, I32, P, P, P, P, P, I32, P, P, P, P], ctypes.c_int),
        "op_haar_candidates": ([P, I32, P, P, P, P, P, I32, P, P, P], ctypes.c_int),
        "op_haar_detect_staged": ([P, P, I32, I32, P, I32, P, P, P, P], ctypes.c_int),
        "op_haar_probe": ([P, P, I32, I32, I64, I32, P, P, P, P, P, P, P, P, P], ctypes.c_int),
        "op_haar_last_ms": ([I32, P], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def build_info():
    """The provenance baked into the loaded library at build time: "sha256:<hex>;defs=<flags>" --
    the digest of its sources and the build flags beyond csrc/Makefile's own (empty for the
    product library)."""
    buf = ctypes.create_string_buffer(1024)
    check(lib().op_build_info(buf, len(buf)), "op_build_info")
    return buf.value.decode("ascii")


def build_digest():
    """The source-digest part of build_info() ("sha256:<hex>")."""
    return build_info().split(";", 1)[0]


def build_flags():
    """The build-flags part of build_info(): "" for the product library."""
    info = build_info()
    return info.split(";defs=", 1)[1] if ";defs=" in info else ""


def check_provenance():
    """Assert the loaded library is the product build of this tree: its source digest equals the
    checked-out sources' and it was built without extra flags.  Returns the digest, or None when
    the sources are absent (an install without csrc/: the digest cannot be verified, nor refuted)."""
    flags = build_flags()
    assert flags == "", "libopenpose_hip.so is an experiment build (flags %r): rebuild the product library" % flags
    tree = source_digest()
    if tree is None:
        return None
    built = build_digest()
    assert built == tree, "libopenpose_hip.so digest %s != sources %s: rebuild it" % (built, tree)
    return built


def source_digest(csrc=None):
    """The same digest recomputed from the checked-out sources (csrc/Makefile DIGEST_SRCS: sha256
    of the `sha256sum` listing of csrc/*.hip *.hpp *.cpp, csrc/Makefile and include/*.h, paths as
    written relative to csrc/, in sorted order); None when the sources are not present."""
    import glob
    import hashlib
    csrc = csrc or os.path.join(_HERE, "csrc")
    if not os.path.isfile(os.path.join(csrc, "Makefile")):
        return None
    names = ["Makefile"]
    for pat in ("*.hip", "*.hpp", "*.cpp"):
        names += [os.path.basename(p) for p in glob.glob(os.path.join(csrc, pat))]
    names += ["../../include/" + os.path.basename(p) for p in glob.glob(os.path.join(csrc, "..", "..", "include", "*.h"))]
    listing = ""
    for n in sorted(names, key=lambda v: v.encode()):
        with open(os.path.join(csrc, n), "rb") as f:
            listing += "%s  %s\n" % (hashlib.sha256(f.read()).hexdigest(), n)
    return "sha256:" + hashlib.sha256(listing.encode()).hexdigest()


def last_error():
    return (lib().op_last_error() or b"").decode("utf-8", "replace")


def check(rc, what=""):
    if rc == OP_OK:
        return
    msg = "%s: %s" % (what, last_error()) if what else last_error()
    if rc == OP_ERR_INDEX:
        raise IndexError("list assignment index out of range")
    if rc == OP_ERR_INVALID:
        raise ValueError(msg)
    if rc == OP_ERR_TIMEOUT:
        raise TimeoutError(msg)
    raise RuntimeError("%s (status %d)" % (msg, rc))


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def default_params():
    p = OpParams()
    check(lib().op_default_params(ctypes.byref(p)))
    return p


def params_from_dict(d):
    p = default_params()
    for k in ("inference_img_size", "heatmap_size", "n_integ_points", "n_integ_points_thresh",
              "n_subset_limbs_thresh", "downscale"):
        if k in d:
            setattr(p, k, int(d[k]))
    for k in ("gaussian_sigma", "heatmap_peak_thresh", "inner_product_thresh", "limb_length_ratio",
              "length_penalty_value", "subset_score_thresh"):
        if k in d:
            setattr(p, k, float(d[k]))
    if "inference_scales" in d:
        sc = list(d["inference_scales"])
        if not 1 <= len(sc) <= MAX_SCALES:
            raise ValueError("inference_scales: 1..%d entries" % MAX_SCALES)
        p.n_scales = len(sc)
        for i, v in enumerate(sc):
            p.inference_scales[i] = float(v)
    if "limbs_point" in d:
        for i, (a, b) in enumerate(d["limbs_point"]):
            p.limbs_point[i][0] = int(a)
            p.limbs_point[i][1] = int(b)
    return p


def layer_table():
    """[(name, ci, co, k)] in models/CocoPoseNet.py:26-129 order, from the library."""
    out = []
    name = ctypes.c_char_p()
    ci, co, k = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    for i in range(N_LAYERS):
        check(lib().op_layer_info(i, ctypes.byref(name), ctypes.byref(ci), ctypes.byref(co), ctypes.byref(k)))
        out.append((name.value.decode(), ci.value, co.value, k.value))
    return out


N_PROBE_POINTS = 46


def probe_table():
    """[(name, channels, divisor)] of op_forward_probe's points 0 .. 45, from the library: the point's
    tensor is (frames, channels, h / divisor, w / divisor)."""
    out = []
    name = ctypes.c_char_p()
    ch, div = ctypes.c_int32(), ctypes.c_int32()
    for i in range(N_PROBE_POINTS):
        check(lib().op_forward_probe_info(i, ctypes.byref(name), ctypes.byref(ch), ctypes.byref(div)),
              "op_forward_probe_info")
        out.append((name.value.decode(), ch.value, div.value))
    return out


N_TRAIN_BUFFERS = 89


def train_buffer_table():
    """[(name, channels, divisor)] of the training step's activation buffers (op_train_buffer_info):
    buffer i is (n, channels, h / divisor, w / divisor), physical channels."""
    out = []
    name = ctypes.c_char_p()
    ch, div = ctypes.c_int32(), ctypes.c_int32()
    for i in range(N_TRAIN_BUFFERS):
        check(lib().op_train_buffer_info(i, ctypes.byref(name), ctypes.byref(ch), ctypes.byref(div)),
              "op_train_buffer_info")
        out.append((name.value.decode(), ch.value, div.value))
    return out


CENSUS = {"7x7_splitk": 11, "7x7_other": 12, "3x3_w48": 13, "3x3_w32": 14, "3x3_pool": 15, "3x3_splitk": 16,
          "3x3_big": 17, "conv1_pair": 18, "3x3_r256": 19, "3x3_r128": 20, "3x3_r_pool": 21,
          "7x7_planar": 22, "7x7_frame_aligned": 23, "7x7_tight": 24,
          "cubic_fused": 25, "cubic_two_pass": 26,
          "cubic_rows": 28, "f32_lds": 29, "7x7_stag": 30, "7x7_plain_ring": 31,
          "7x7_q": 32, "7x7_circ": 33, "precise_side": 34, "7x7_q_iwg": 35, "7x7_lin": 36, "7x7_q_bpf": 37, "7x7_pers": 38}
CENSUS_SLOTS = 40


def conv_census(reset=False):
    """Process-wide launch counts of the bf16x3 conv kernels (op_conv_census): {"npx": {NPX: n}
    for the 7x7 raster kernel, plus the CENSUS slots by name}."""
    a = (ctypes.c_int32 * CENSUS_SLOTS)()
    check(lib().op_conv_census(a, CENSUS_SLOTS, 1 if reset else 0), "op_conv_census")
    out = {"npx": {i: a[i] for i in range(1, 11) if a[i]}}
    out.update({k: a[v] for k, v in CENSUS.items()})
    return out


def forward_flops(h, w):
    return float(lib().op_forward_flops(int(h), int(w)))


class Context(object):
    """Owns one op_ctx (one device, one stream, packed weights in HBM)."""

    def __init__(self, device=0, params=None, limits=None):
        L = lib()
        self._p = params if params is not None else default_params()
        self._l = limits if limits is not None else OpLimits()
        h = ctypes.c_void_p()
        check(L.op_create(ctypes.byref(self._p), ctypes.byref(self._l), int(device), ctypes.byref(h)), "op_create")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            lib().op_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_precision(self, mode):
        """'bf16x3' (default: 3xBF16 split products, f32 accumulate) or 'fp32' (exact f32 MFMA)."""
        check(lib().op_set_precision(self.h, PRECISION[mode]), "op_set_precision")

    def get_precision(self):
        m = ctypes.c_int32()
        check(lib().op_get_precision(self.h, ctypes.byref(m)), "op_get_precision")
        return {v: k for k, v in PRECISION.items()}[m.value]

    def set_weights(self, weights):
        """weights: {layer name: (W (Co,Ci,k,k) f32, b (Co,) f32)}."""
        table = layer_table()
        keep = []
        Wp = (ctypes.c_void_p * N_LAYERS)()
        bp = (ctypes.c_void_p * N_LAYERS)()
        for i, (name, ci, co, k) in enumerate(table):
            if name not in weights:
                raise KeyError("missing weights for layer %s" % name)
            W, b = weights[name]
            W = np.ascontiguousarray(W, dtype=np.float32)
            b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
            if W.shape != (co, ci, k, k) or b.shape != (co,):
                raise ValueError("layer %s: expected W%s b(%d,), got %s %s" % (name, (co, ci, k, k), co, W.shape, b.shape))
            keep += [W, b]
            Wp[i] = W.ctypes.data
            bp[i] = b.ctypes.data
        check(lib().op_set_weights(self.h, Wp, bp), "op_set_weights")

    # ---- results ----
    def _result_arrays(self, cap):
        return np.empty((cap, N_JOINTS, 3), np.float64), np.empty(cap, np.float64), OpFrameResult()

    def detect(self, img, cap=2048):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("expected an H x W x 3 uint8 BGR image")
        poses, scores, res = self._result_arrays(cap)
        rc = lib().op_detect(self.h, ptr(img), img.shape[0], img.shape[1], img.strides[0], ptr(poses), ptr(scores),
                             cap, ctypes.byref(res))
        if rc == OP_ERR_CAPACITY and res.n_persons > cap:  # more persons than rows: the frame stays staged
            return self.fetch_result(0, cap=res.n_persons)
        check(rc, "op_detect")
        return poses[:res.n_persons].copy(), scores[:res.n_persons].copy(), res

    def set_conv_algo(self, algo):
        """Kernel family of the bf16x3 convolutions (include/openpose_hip.h: op_set_conv_algo)."""
        check(lib().op_set_conv_algo(self.h, int(algo)), "op_set_conv_algo")

    def set_stage_layout(self, planar):
        """Chunk-planar (1, default) or [row][col][channels] (0) 7x7 stage tensors
        (include/openpose_hip.h: op_set_stage_layout); the maps are bit-identical either way."""
        check(lib().op_set_stage_layout(self.h, 1 if planar else 0), "op_set_stage_layout")

    def set_peak_mode(self, branch="cpu", ksize=None):
        """Peak semantics of the single-scale post-process (include/openpose_hip.h: op_set_peak_mode):
        'cpu' (default; pose_detector.py:82-110) or 'gpu', the reference's GPU branch
        (pose_detector.py:111-132: ksize x ksize unnormalised Gaussian with zero padding, >= NMS;
        ksize defaults to params['ksize'] = 17)."""
        if branch not in PEAK_BRANCH:
            raise ValueError("peak branch %r: 'cpu' or 'gpu'" % (branch,))
        k = int(ksize if ksize is not None else 17)
        check(lib().op_set_peak_mode(self.h, PEAK_BRANCH[branch], k), "op_set_peak_mode")

    def set_batch_invariant(self, enable=True):
        """One accumulation order for every batch size (include/openpose_hip.h: op_set_batch_invariant);
        off by default: lone frames split their 7x7 input channels over workgroups (~2x lower latency)."""
        check(lib().op_set_batch_invariant(self.h, int(bool(enable))), "op_set_batch_invariant")

    def detect_precise(self, img, cap=2048, return_maps=False):
        """detect_precise (pose_detector.py:433-482): (poses, scores, res[, pafs (38,h,w), heatmaps (19,h,w)])."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("expected an H x W x 3 uint8 BGR image")
        h, w = img.shape[:2]
        poses, scores, res = self._result_arrays(cap)
        pafs = np.empty((N_PAF, h, w), np.float32) if return_maps else None
        heat = np.empty((N_HEAT, h, w), np.float32) if return_maps else None
        rc = lib().op_detect_precise(self.h, ptr(img), h, w, img.strides[0], ptr(poses), ptr(scores), cap,
                                     ctypes.byref(res), ptr(pafs) if return_maps else None,
                                     ptr(heat) if return_maps else None)
        if rc == OP_ERR_CAPACITY and res.n_persons > cap:  # more persons than rows: the frame stays staged
            out = self.fetch_result(0, cap=res.n_persons)
            return out + (pafs, heat) if return_maps else out
        try:
            check(rc, "op_detect_precise")
        except IndexError as e:  # the averaged maps are valid: keep them for inspection
            e.maps = (pafs, heat)
            raise
        out = (poses[:res.n_persons].copy(), scores[:res.n_persons].copy(), res)
        return out + (pafs, heat) if return_maps else out

    def resize_cubic(self, img, out_w, out_h):
        """cv2.resize(img, (out_w, out_h), interpolation=cv2.INTER_CUBIC) for uint8 / float32 H x W (x C)."""
        a = np.asarray(img)
        if a.dtype == np.uint8:
            dt = 0
        elif a.dtype == np.float32:
            dt = 1
        else:
            raise ValueError("uint8 or float32 image expected")
        a = np.ascontiguousarray(a)
        cn = 1 if a.ndim == 2 else a.shape[2]
        out = np.empty((out_h, out_w, cn), a.dtype)
        check(lib().op_resize_cubic(self.h, ptr(a), dt, a.shape[0], a.shape[1], cn, ptr(out), out_h, out_w),
              "op_resize_cubic")
        return out if a.ndim == 3 else out[:, :, 0]

    def preprocess(self, img, out_w, out_h):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        x = np.empty((1, 3, out_h, out_w), np.float32)
        check(lib().op_preprocess(self.h, ptr(img), img.shape[0], img.shape[1], img.strides[0], out_w, out_h, ptr(x)),
              "op_preprocess")
        return x

    def forward(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        n, c, h, w = x.shape
        if c != 3:
            raise ValueError("expected (n, 3, h, w)")
        paf = np.empty((n, N_PAF, h // 8, w // 8), np.float32)
        heat = np.empty((n, N_HEAT, h // 8, w // 8), np.float32)
        check(lib().op_forward(self.h, ptr(x), n, h, w, ptr(paf), ptr(heat)), "op_forward")
        return paf, heat

    def forward_stages(self, x):
        """All six stages: pafs (6, n, 38, h/8, w/8), heatmaps (6, n, 19, h/8, w/8)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n, c, h, w = x.shape
        if c != 3:
            raise ValueError("expected (n, 3, h, w)")
        paf = np.empty((6, n, N_PAF, h // 8, w // 8), np.float32)
        heat = np.empty((6, n, N_HEAT, h // 8, w // 8), np.float32)
        check(lib().op_forward_stages(self.h, ptr(x), n, h, w, ptr(paf), ptr(heat)), "op_forward_stages")
        return paf, heat

    def forward_probe(self, x, point, frames=None):
        """What probe point `point` of the forward wrote (include/openpose_hip.h: op_forward_probe), as
        dense f32 (frames, channels, h / divisor, w / divisor); frames = (first, count), default all."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n, c, h, w = x.shape
        if c != 3:
            raise ValueError("expected (n, 3, h, w)")
        f0, nf = (0, n) if frames is None else (int(frames[0]), int(frames[1]))
        name, ch, div = ctypes.c_char_p(), ctypes.c_int32(), ctypes.c_int32()
        check(lib().op_forward_probe_info(int(point), ctypes.byref(name), ctypes.byref(ch), ctypes.byref(div)),
              "op_forward_probe_info")
        out = np.empty((max(nf, 0), ch.value, h // div.value, w // div.value), np.float32)
        check(lib().op_forward_probe(self.h, ptr(x), n, h, w, int(point), f0, nf, ptr(out), out.size), "op_forward_probe")
        return out

    def resize_images(self, x, oh, ow):
        x = np.ascontiguousarray(x, dtype=np.float32)
        c, h, w = x.shape
        y = np.empty((c, oh, ow), np.float32)
        check(lib().op_resize_images(self.h, ptr(x), c, h, w, oh, ow, ptr(y)), "op_resize_images")
        return y

    def compute_peaks(self, heatmaps):
        heatmaps = np.ascontiguousarray(heatmaps, dtype=np.float32)
        c, h, w = heatmaps.shape
        cap = max(1, N_JOINTS * 2048)
        while True:  # uncapped: on a too-small array the library reports the rows it needs
            out = np.empty((cap, 5), np.float64)
            n = ctypes.c_int64()
            rc = lib().op_compute_peaks(self.h, ptr(heatmaps), c, h, w, ptr(out), cap, ctypes.byref(n))
            if rc == OP_ERR_CAPACITY and n.value > cap:
                cap = n.value
                continue
            check(rc, "op_compute_peaks")
            return out[:n.value].copy()

    def compute_connections(self, pafs, peaks, img_len):
        pafs = np.ascontiguousarray(pafs, dtype=np.float32)
        peaks = np.ascontiguousarray(np.asarray(peaks, np.float64).reshape(-1, 5))
        _, h, w = pafs.shape
        cap = max(1, N_LIMBS * 2048)
        while True:
            conn = np.empty((cap, 3), np.float64)
            off = np.zeros(N_LIMBS + 1, np.int64)
            rc = lib().op_compute_connections(self.h, ptr(pafs), h, w, ptr(peaks), len(peaks), float(img_len),
                                              ptr(conn), cap, ptr(off))
            if rc == OP_ERR_CAPACITY and off[N_LIMBS] > cap:
                cap = int(off[N_LIMBS])
                continue
            check(rc, "op_compute_connections")
            return [conn[off[l]:off[l + 1]].copy() for l in range(N_LIMBS)]

    def grouping(self, connections, peaks):
        peaks = np.ascontiguousarray(np.asarray(peaks, np.float64).reshape(-1, 5))
        rows = [np.asarray(c, np.float64).reshape(-1, 3) for c in connections]
        conn = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 3)))
        off = np.zeros(N_LIMBS + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in rows])
        cap = 2048
        cptr = conn if len(conn) else np.zeros((1, 3))
        while True:
            subsets = np.empty((cap, 20), np.float64)
            n = ctypes.c_int64()
            rc = lib().op_grouping(self.h, ptr(cptr), ptr(off), ptr(peaks), len(peaks), ptr(subsets), cap,
                                   ctypes.byref(n))
            if rc == OP_ERR_CAPACITY and n.value > cap:
                cap = n.value
                continue
            check(rc, "op_grouping")
            return subsets[:n.value].copy()

    def postprocess(self, paf_low, heat_low, orig_h, orig_w, cap=2048):
        paf_low = np.ascontiguousarray(paf_low, dtype=np.float32)
        heat_low = np.ascontiguousarray(heat_low, dtype=np.float32)
        _, h, w = paf_low.shape
        while True:
            poses, scores, res = self._result_arrays(cap)
            rc = lib().op_postprocess(self.h, ptr(paf_low), ptr(heat_low), h, w, int(orig_h), int(orig_w),
                                      ptr(poses), ptr(scores), cap, ctypes.byref(res))
            if rc == OP_ERR_CAPACITY and res.n_persons > cap:
                cap = res.n_persons
                continue
            check(rc, "op_postprocess")
            return poses[:res.n_persons].copy(), scores[:res.n_persons].copy(), res

    # ---- staged batched path ----
    def stage_frames(self, frames):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n, h, w, c = frames.shape
        check(lib().op_stage_frames(self.h, ptr(frames), n, h, w), "op_stage_frames")

    def stage_jpegs(self, datas, h, w, bgr=None):
        """Stage files instead of pixels (op_jpeg_stage): frame f from ``bgr[f]`` ((h, w, 3) uint8) where
        that is given, else decoded on the device from ``datas[f]`` (bytes) straight into the staged
        set -> the per-frame OP_JPEG_* statuses (a frame with a non-zero status is staged as zeros)."""
        n = len(datas)
        bgr = list(bgr) if bgr is not None else [None] * n
        if len(bgr) != n:
            raise ValueError("Context.stage_jpegs: %d files, %d bgr entries" % (n, len(bgr)))
        keep = [np.ascontiguousarray(b, dtype=np.uint8) if b is not None else None for b in bgr]
        for b in keep:
            if b is not None and b.shape != (h, w, 3):
                raise ValueError("Context.stage_jpegs: a bgr frame of shape %r, not (%d, %d, 3)" % (b.shape, h, w))
        files, data_p, size_p = _jpeg_files([d if k is None else None for d, k in zip(datas, keep)])
        bgr_p = (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data if b is not None else None for b in keep])
        status = np.zeros(max(n, 1), np.int32)
        check(lib().op_jpeg_stage(self.h, n, data_p, size_p, bgr_p, int(h), int(w), ptr(status)), "op_jpeg_stage")
        return status[:n]

    def upload_frames(self, frames):
        """Asynchronous staging (op_upload_frames): the next run_staged* uses these frames; keep
        `frames` (ideally a PinnedFrames array) unchanged until the copy has completed
        (upload_wait(), synchronize(), or a later call that waited for the consuming run)."""
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or not frames.flags.c_contiguous:
            raise ValueError("expected contiguous (n, h, w, 3) uint8 frames")
        n, h, w, _ = frames.shape
        check(lib().op_upload_frames(self.h, ctypes.c_void_p(frames.ctypes.data), n, h, w), "op_upload_frames")

    def upload_wait(self):
        """Block until every upload_frames copy has finished reading its host buffer."""
        check(lib().op_upload_wait(self.h), "op_upload_wait")

    def stage_maps(self, maps):
        maps = np.ascontiguousarray(maps, dtype=np.float32)
        n, c, h, w = maps.shape
        if c != N_PAF + N_HEAT:
            raise ValueError("maps must be (n, 57, h, w): 38 PAF then 19 heatmap channels")
        check(lib().op_stage_maps(self.h, ptr(maps), n, h, w), "op_stage_maps")

    def use_staged_maps(self, enable):
        check(lib().op_use_staged_maps(self.h, 1 if enable else 0))

    def staged_info(self):
        """(n, h, w) of the staged frame set, (0, 0, 0) when nothing is staged (op_staged_info)."""
        v = [ctypes.c_int32() for _ in range(3)]
        check(lib().op_staged_info(self.h, *[ctypes.byref(x) for x in v]), "op_staged_info")
        return tuple(x.value for x in v)

    def run_staged(self, graph=False):
        check((lib().op_run_staged_graph if graph else lib().op_run_staged)(self.h), "op_run_staged")

    def run_staged_precise(self):
        """detect_precise on every staged frame (batched per scale; op_run_staged_precise)."""
        check(lib().op_run_staged_precise(self.h), "op_run_staged_precise")

    def synchronize(self):
        check(lib().op_synchronize(self.h), "op_synchronize")

    def graph_info(self):
        """Node counts of the last captured step graph (op_graph_info)."""
        v = [ctypes.c_int32() for _ in range(5)]
        check(lib().op_graph_info(self.h, *[ctypes.byref(x) for x in v]), "op_graph_info")
        return dict(zip(("nodes", "kernels", "memsets", "memcpys", "host_nodes"), (x.value for x in v)))

    def fetch_result(self, frame, cap=2048):
        while True:
            poses, scores, res = self._result_arrays(cap)
            rc = lib().op_fetch_result(self.h, int(frame), ptr(poses), ptr(scores), cap, ctypes.byref(res))
            if rc == OP_ERR_CAPACITY and res.n_persons > cap:
                cap = res.n_persons
                continue
            check(rc, "op_fetch_result")
            return poses[:res.n_persons].copy(), scores[:res.n_persons].copy(), res

    def fetch_results(self, first, n, cap=64):
        """Results of staged frames [first, first+n) in three copies: [(poses, scores, res), ...]."""
        while True:
            poses = np.empty((n, cap, N_JOINTS, 3), np.float64)
            scores = np.empty((n, cap), np.float64)
            res = (OpFrameResult * n)()
            rc = lib().op_fetch_results(self.h, int(first), int(n), ptr(poses), ptr(scores), cap, res)
            most = max(r.n_persons for r in res)
            if rc == OP_ERR_CAPACITY and most > cap:
                cap = most
                continue
            check(rc, "op_fetch_results")
            break
        return [(poses[i, :res[i].n_persons].copy(), scores[i, :res[i].n_persons].copy(), res[i]) for i in range(n)]

    def body_rois(self, first, n, cap=64):
        """Face / hand boxes of the persons of staged frames [first, first + n), made on the device
        from the result rows where they lie (op_body_rois_staged; wholebody.body_rois_np states them):
        -> (count (n,), frame_status (n,), unit (n, cap), box (n, cap, 3, 4), state (n, cap, 3)); the
        persons of frame i are rows [:min(count[i], cap)].  A frame with more persons than ``cap`` raises
        nothing here: its ``count`` says so and the caller takes it through ``fetch_result`` and
        ``_lib.body_rois`` (as it does a frame whose ``frame_status`` is OP_ERR_CAPACITY)."""
        n, cap = int(n), int(cap)
        count = np.zeros(max(n, 1), np.int32)
        status = np.zeros(max(n, 1), np.int32)
        unit = np.zeros((max(n, 1), max(cap, 1)), np.float64)
        box = np.zeros((max(n, 1), max(cap, 1), 3, 4), np.int32)
        state = np.zeros((max(n, 1), max(cap, 1), 3), np.int32)
        rc = lib().op_body_rois_staged(self.h, int(first), n, cap, ptr(count), ptr(status), ptr(unit), ptr(box),
                                       ptr(state))
        if not (rc == OP_ERR_CAPACITY and count.max() > cap):
            check(rc, "op_body_rois_staged")
        return count, status, unit, box, state

    def keypoint_match(self, first, n, gts, joint_map=None, max_dets=None, thrs=None, area_rng=None, sigmas=None,
                       want_oks=False):
        """COCO keypoint matching of the persons of staged frames [first, first + n) against ``gts``
        (per frame ``keypoint_eval.gt_tables``' tuple), on the device from the result rows where they
        lie (op_keypoint_match_staged; keypoint_eval.match_np states it) -> (frame_status (n,), the
        list of per-frame records).  A frame whose status is not OP_OK comes back with no detections:
        the caller takes it through ``fetch_result`` and ``_lib.keypoint_match``."""
        from . import keypoint_eval as K
        n = int(n)
        if len(gts) != n:
            raise ValueError("Context.keypoint_match: %d frames, %d ground-truth tables" % (n, len(gts)))
        g = _KeypointCall(gts, max_dets, thrs, area_rng, sigmas, want_oks)
        jm = np.ascontiguousarray(K.joint_map() if joint_map is None else joint_map, np.int32)
        if jm.shape != (17,):
            raise ValueError("Context.keypoint_match: joint_map has 17 entries")
        status = np.zeros(max(n, 1), np.int32)
        count = np.zeros(max(n, 1), np.int32)
        scores = np.zeros((max(n, 1), g.M), np.float64)
        g.outputs(n)
        check(lib().op_keypoint_match_staged(self.h, int(first), n, ptr(jm), *(g.gt_args() + g.const_args() + [
            ptr(status), ptr(count), ptr(scores)] + g.out_args())), "op_keypoint_match_staged")
        return status[:n], g.records(n, [scores[i, :min(int(count[i]), g.M)].copy() for i in range(n)])

    def fetch_maps(self, first=0, n=1):
        """Network maps of staged frames [first, first+n): (pafs (n,38,h,w), heatmaps (n,19,h,w)) --
        the last-stage maps of run_staged, or the averaged full-resolution maps of run_staged_precise."""
        mh, mw = ctypes.c_int32(), ctypes.c_int32()
        check(lib().op_fetch_maps(self.h, int(first), int(n), None, None, ctypes.byref(mh), ctypes.byref(mw)),
              "op_fetch_maps")
        pafs = np.empty((n, N_PAF, mh.value, mw.value), np.float32)
        heat = np.empty((n, N_HEAT, mh.value, mw.value), np.float32)
        check(lib().op_fetch_maps(self.h, int(first), int(n), ptr(pafs), ptr(heat), ctypes.byref(mh),
                                  ctypes.byref(mw)), "op_fetch_maps")
        return pafs, heat

    def last_timing(self):
        a, b, t = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(lib().op_last_timing(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(t)), "op_last_timing")
        return a.value, b.value, t.value

    # ---- per-kernel-class event timing ----
    PROFILE_CLASSES = ("conv7x7", "conv3x3", "conv1x1", "postprocess", "input", "map_resize", "other")

    def profile(self, enable=True):
        check(lib().op_profile_enable(self.h, 1 if enable else 0), "op_profile_enable")

    def profile_classes(self, names):
        """Time only these classes (names from PROFILE_CLASSES) while profiling is enabled."""
        mask = 0
        for n in names:
            mask |= 1 << self.PROFILE_CLASSES.index(n)
        check(lib().op_profile_classes(self.h, mask), "op_profile_classes")

    def profile_reset(self):
        check(lib().op_profile_reset(self.h), "op_profile_reset")

    def profile_read(self):
        """{class: (ms, launches, algorithmic flops, algorithmic bytes)} since the last reset."""
        out = {}
        for i, name in enumerate(self.PROFILE_CLASSES):
            ms, n, fl, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            check(lib().op_profile_read(self.h, i, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl),
                                        ctypes.byref(by)), "op_profile_read")
            out[name] = (ms.value, n.value, fl.value, by.value)
        return out


def _jpeg_files(datas):
    """-> (the buffers kept alive, a void* array of their addresses (null for None), an int64 array of sizes)."""
    files = [np.frombuffer(d, np.uint8) if d is not None and len(d) else None for d in datas]
    empty = np.zeros(1, np.uint8)  # an empty file still has an address
    addr = [(f if f is not None else empty).ctypes.data if d is not None else None for f, d in zip(files, datas)]
    data_p = (ctypes.c_void_p * max(len(datas), 1))(*addr)
    size_p = (ctypes.c_int64 * max(len(datas), 1))(*[len(d) if d is not None else 0 for d in datas])
    return (files, empty), data_p, size_p


def jpeg_probe(data):
    """op_jpeg_probe -> OpJpegInfo (headers only, on the host)."""
    info = OpJpegInfo()
    keep, data_p, size_p = _jpeg_files([data])
    check(lib().op_jpeg_probe(data_p[0], size_p[0], ctypes.byref(info)), "op_jpeg_probe")
    return info


def jpeg_coefficients(data):
    """op_jpeg_coefficients -> (status, info, coef (n_blocks, 64) int16, qt (3, 64) uint16): the host's
    entropy decode of one file (jpeg.coefficients_np states it)."""
    info = jpeg_probe(data)
    coef = np.zeros((max(int(info.n_blocks), 1), 64), np.int16)
    qt = np.zeros((3, 64), np.uint16)
    status = ctypes.c_int32(-1)
    keep, data_p, size_p = _jpeg_files([data])
    check(lib().op_jpeg_coefficients(data_p[0], size_p[0], ptr(coef), coef.size, ptr(qt), ctypes.byref(status)),
          "op_jpeg_coefficients")
    return status.value, info, coef[:int(info.n_blocks)], qt


def jpeg_block_in_range(coef, q):
    coef = np.ascontiguousarray(coef, np.int16).reshape(64)
    q = np.ascontiguousarray(q, np.uint16).reshape(64)
    out = ctypes.c_int32(-1)
    check(lib().op_jpeg_block_in_range(ptr(coef), ptr(q), ctypes.byref(out)), "op_jpeg_block_in_range")
    return bool(out.value)


def jpeg_decode(datas, outs, device=0):
    """op_jpeg_decode: ``outs[f]`` a contiguous (h, w, 3) uint8 array (or None for a frame the probe
    turned down) -> statuses (n,) int32."""
    n = len(datas)
    keep, data_p, size_p = _jpeg_files(datas)
    out_p = (ctypes.c_void_p * max(n, 1))(*[o.ctypes.data if o is not None else None for o in outs])
    status = np.zeros(max(n, 1), np.int32)
    check(lib().op_jpeg_decode(int(device), n, data_p, size_p, out_p, ptr(status)), "op_jpeg_decode")
    return status[:n]


def jpeg_set_threads(threads):
    """Threads of the entropy-decode pool (op_jpeg_set_threads): 1 .. 64, 0 for the default again."""
    check(lib().op_jpeg_set_threads(int(threads)), "op_jpeg_set_threads")


def jpeg_last_ms(device=0):
    """(host entropy-decode ms, device ms) of the last op_jpeg_decode / op_jpeg_stage on ``device``."""
    ms = (ctypes.c_double * 2)()
    check(lib().op_jpeg_last_ms(int(device), ms), "op_jpeg_last_ms")
    return ms[0], ms[1]


def haar_params(scale_factor=1.2, min_neighbors=3, min_size=(1, 1), max_size=None, max_candidates=0):
    """-> OpHaarParams; sizes are (w, h) as in cv2."""
    p = OpHaarParams()
    p.scale_factor, p.min_neighbors = float(scale_factor), int(min_neighbors)
    p.min_w, p.min_h = int(min_size[0]), int(min_size[1])
    p.has_max = 0 if max_size is None else 1
    p.max_w, p.max_h = (0, 0) if max_size is None else (int(max_size[0]), int(max_size[1]))
    p.max_candidates = int(max_candidates)
    return p


class HaarHandle(object):
    """An op_haar: a cascade (haar.load_cascade's dict) uploaded to ``device``."""

    def __init__(self, cascade, device=0):
        self.h = ctypes.c_void_p()
        self.device = int(device)
        kinds = dict(stage_first=np.int32, rects=np.int32, win=np.int32)
        c = {k: np.ascontiguousarray(v, kinds.get(k, np.float32)) for k, v in cascade.items()}  # alive through the call
        self.win = (int(c["win"][0]), int(c["win"][1]))
        self.n_stages = len(c["stage_thr"])
        check(lib().op_haar_create(self.device, self.win[0], self.win[1], self.n_stages, ptr(c["stage_first"]),
                                   ptr(c["stage_thr"]), len(c["thr"]), ptr(c["rects"]), ptr(c["weights"]), ptr(c["thr"]),
                                   ptr(c["left"]), ptr(c["right"]), ctypes.byref(self.h)), "op_haar_create")

    def close(self):
        if self.h:
            lib().op_haar_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _frames(frames):
        """-> (arrays kept alive, bgr void*[], hw int32, row_stride int64, channels int32)"""
        keep = []
        for f in frames:
            f = np.asarray(f)
            if f.dtype != np.uint8 or f.ndim not in (2, 3) or (f.ndim == 3 and f.shape[2] != 3):
                raise ValueError("a frame is (h, w) or (h, w, 3) uint8, not %s %s" % (f.dtype, f.shape))
            if f.strides[1:] != ((3, 1) if f.ndim == 3 else (1,)) or f.strides[0] < f.shape[1] * (3 if f.ndim == 3 else 1):
                f = np.ascontiguousarray(f)
            keep.append(f)
        n = len(keep)
        bgr = (ctypes.c_void_p * max(n, 1))(*[f.ctypes.data for f in keep])
        hw = np.array([[f.shape[0], f.shape[1]] for f in keep], np.int32).reshape(-1, 2)
        stride = np.array([f.strides[0] for f in keep], np.int64)
        channels = np.array([3 if f.ndim == 3 else 1 for f in keep], np.int32)
        return keep, bgr, hw, stride, channels

    def detect(self, frames, scale_factor=1.2, min_neighbors=3, min_size=(1, 1), max_size=None, max_candidates=0, cap=64):
        """op_haar_detect -> (rects (n, cap, 4), neighbours (n, cap), count (n,), status (n,)) int32: frame f
        has count[f] rectangles when status[f] is OP_OK; OP_ERR_CAPACITY: count[f] is what it needs."""
        keep, bgr, hw, stride, channels = self._frames(frames)
        n = len(keep)
        prm = haar_params(scale_factor, min_neighbors, min_size, max_size, max_candidates)
        rects, neigh = np.zeros((n, cap, 4), np.int32), np.zeros((n, cap), np.int32)
        count, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        check(lib().op_haar_detect(self.h, n, bgr, ptr(hw), ptr(stride), ptr(channels), ctypes.byref(prm), int(cap),
                                   ptr(rects), ptr(neigh), ptr(count), ptr(status)), "op_haar_detect")
        return rects, neigh, count, status

    def candidates(self, frames, scale_factor=1.2, min_size=(1, 1), max_size=None, max_candidates=0, cap=4096):
        """op_haar_candidates -> (rects (n, cap, 4), count (n,), status (n,))."""
        keep, bgr, hw, stride, channels = self._frames(frames)
        n = len(keep)
        prm = haar_params(scale_factor, 0, min_size, max_size, max_candidates)
        rects = np.zeros((n, cap, 4), np.int32)
        count, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        check(lib().op_haar_candidates(self.h, n, bgr, ptr(hw), ptr(stride), ptr(channels), ctypes.byref(prm), int(cap),
                                       ptr(rects), ptr(count), ptr(status)), "op_haar_candidates")
        return rects, count, status

    def detect_staged(self, ctx, first, n, scale_factor=1.2, min_neighbors=3, min_size=(1, 1), max_size=None,
                      max_candidates=0, cap=64):
        """op_haar_detect_staged on frames [first, first + n) of ``ctx`` (a Context): as ``detect``."""
        prm = haar_params(scale_factor, min_neighbors, min_size, max_size, max_candidates)
        m = max(int(n), 0)
        rects, neigh = np.zeros((m, cap, 4), np.int32), np.zeros((m, cap), np.int32)
        count, status = np.zeros(m, np.int32), np.zeros(m, np.int32)
        check(lib().op_haar_detect_staged(self.h, ctx.h, int(first), int(n), ctypes.byref(prm), int(cap), ptr(rects),
                                          ptr(neigh), ptr(count), ptr(status)), "op_haar_detect_staged")
        return rects, neigh, count, status

    def probe(self, frame, scale_factor=1.2, min_size=(1, 1), max_size=None):
        """op_haar_probe -> [dict(scale, pixels, sum, sqsum, map)] per layer, what haar.result_map_np and
        haar.pyramid_np state."""
        keep, bgr, hw, stride, channels = self._frames([frame])
        prm = haar_params(scale_factor, 0, min_size, max_size, 0)
        nl = ctypes.c_int32(0)
        lhw, lsc = np.zeros((HAAR_MAX_SCALES, 2), np.int32), np.zeros(HAAR_MAX_SCALES, np.float32)

        def call(pix, s, q, m, cap):
            check(lib().op_haar_probe(self.h, bgr[0], int(hw[0, 0]), int(hw[0, 1]), int(stride[0]), int(channels[0]),
                                      ctypes.byref(prm), ctypes.byref(nl), ptr(lhw), ptr(lsc), ptr(pix), ptr(s), ptr(q),
                                      ptr(m), ptr(cap)), "op_haar_probe")
        call(None, None, None, None, None)
        shapes = []
        for i in range(nl.value):
            lh, lw = int(lhw[i, 0]), int(lhw[i, 1])
            step = 1 if float(lsc[i]) >= 2.0 else 2
            shapes.append((lh, lw, len(range(0, lh - self.win[1], step)), len(range(0, lw - self.win[0], step))))
        cap = np.array([sum(a * b for a, b, _, _ in shapes), sum((a + 1) * (b + 1) for a, b, _, _ in shapes),
                        sum(c * d for _, _, c, d in shapes)], np.int64)
        pix, s, q = np.zeros(max(cap[0], 1), np.uint8), np.zeros(max(cap[1], 1), np.int32), np.zeros(max(cap[1], 1), np.uint32)
        m = np.full(max(cap[2], 1), -128, np.int8)
        if nl.value:
            call(pix, s, q, m, cap)
        out, a, b, c = [], 0, 0, 0
        for i, (lh, lw, gy, gx) in enumerate(shapes):
            out.append(dict(scale=lsc[i], pixels=pix[a:a + lh * lw].reshape(lh, lw),
                            sum=s[b:b + (lh + 1) * (lw + 1)].reshape(lh + 1, lw + 1),
                            sqsum=q[b:b + (lh + 1) * (lw + 1)].reshape(lh + 1, lw + 1), map=m[c:c + gy * gx].reshape(gy, gx)))
            a, b, c = a + lh * lw, b + (lh + 1) * (lw + 1), c + gy * gx
        return out


def haar_last_ms(device=0):
    """Device times (ms, stream events) of the last Haar call that completed on ``device``: a dict
    with the keys of HAAR_TIMES (the whole call, then its grey, pyramid, integral and cascade launches)."""
    ms = (ctypes.c_double * len(HAAR_TIMES))()
    check(lib().op_haar_last_ms(int(device), ms), "op_haar_last_ms")
    return dict(zip(HAAR_TIMES, ms))


def body_rois(poses, device=0):
    """Face / hand boxes from poses (P, 18, 3) on the device (op_body_rois), bit-identical to
    wholebody.body_rois_np: -> (unit (P,) f64, box (P, 3, 4) int32 in the order face, left hand, right
    hand as (l, t, r, b), state (P, 3) int32: 0 absent, 1 valid, 2 present but not runnable)."""
    poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, N_JOINTS, 3))
    n = len(poses)
    unit = np.zeros(n, np.float64)
    box = np.zeros((n, 3, 4), np.int32)
    state = np.zeros((n, 3), np.int32)
    if n:
        check(lib().op_body_rois(int(device), n, ptr(poses), ptr(unit), ptr(box), ptr(state)), "op_body_rois")
    return unit, box, state


def body_last_ms(device=0):
    """Device time (upload + kernel, stream events) of the last ``body_rois`` / ``Context.body_rois``
    that completed on this device."""
    ms = ctypes.c_double()
    check(lib().op_body_last_ms(int(device), ctypes.byref(ms)), "op_body_last_ms")
    return ms.value


class _KeypointCall(object):
    """The ground-truth tables, constants and output arrays of one op_keypoint_match* call, and the
    per-frame records (keypoint_eval.match_np's dict) cut out of the outputs."""

    def __init__(self, gts, max_dets, thrs, area_rng, sigmas, want_oks):
        from . import keypoint_eval as K
        self.M = int(K.MAX_DETS if max_dets is None else max_dets)
        self.thrs = np.ascontiguousarray(K.OKS_THRS if thrs is None else thrs, np.float64).reshape(-1)
        self.rng = np.ascontiguousarray(K.AREA_RNG if area_rng is None else area_rng, np.float64).reshape(-1, 2)
        self.sig = np.ascontiguousarray(K.KPT_SIGMAS if sigmas is None else sigmas, np.float64).reshape(-1)
        if self.sig.shape != (17,):
            raise ValueError("keypoint_match: sigmas has 17 entries")
        if not 1 <= self.M <= 64:
            raise ValueError("keypoint_match: max_dets must be in 1 .. 64")
        self.want_oks = bool(want_oks)
        self.T, self.A = len(self.thrs), len(self.rng)
        counts = [len(np.asarray(g[1]).reshape(-1)) for g in gts]
        self.off = np.zeros(len(gts) + 1, np.int32)
        self.off[1:] = np.cumsum(counts)
        G = self.G = int(self.off[-1])

        def cat(k, shape, dtype):
            out = np.zeros((max(G, 1),) + shape, dtype)
            if G:
                out[:G] = np.concatenate([np.asarray(g[k], dtype).reshape((-1,) + shape) for g in gts])
            return out

        self.kpts, self.area, self.bbox = cat(0, (17, 3), np.float64), cat(1, (), np.float64), cat(2, (4,), np.float64)
        self.ignore = cat(3, (), np.uint8) if not G else np.ascontiguousarray(
            np.concatenate([np.asarray(g[3]).reshape(-1) != 0 for g in gts]), np.uint8)
        self.crowd = cat(4, (), np.uint8) if not G else np.ascontiguousarray(
            np.concatenate([np.asarray(g[4]).reshape(-1) != 0 for g in gts]), np.uint8)

    def gt_args(self):
        return [ptr(self.off), ptr(self.kpts), ptr(self.area), ptr(self.bbox), ptr(self.ignore), ptr(self.crowd)]

    def const_args(self):
        return [self.M, self.T, ptr(self.thrs), self.A, ptr(self.rng), ptr(self.sig)]

    def outputs(self, n):
        M, A, T, G = self.M, self.A, self.T, self.G
        self.dt_order = np.full((max(n, 1), M), -1, np.int32)
        self.oks = np.zeros(max(M * G, 1), np.float64) if self.want_oks else None
        self.dt_match = np.full((max(n, 1), A, T, M), -1, np.int32)
        self.dt_ignore = np.zeros((max(n, 1), A, T, M), np.uint8)
        self.gt_match = np.full(max(A * T * G, 1), -1, np.int32)
        self.gt_ig = np.zeros(max(A * G, 1), np.uint8)

    def out_args(self):
        return [ptr(self.dt_order), ptr(self.oks), ptr(self.dt_match), ptr(self.dt_ignore), ptr(self.gt_match),
                ptr(self.gt_ig)]

    def records(self, n, scores):
        """scores: per frame the kept detections' scores, in order."""
        M, A, T = self.M, self.A, self.T
        out = []
        for f in range(n):
            g0, g1 = int(self.off[f]), int(self.off[f + 1])
            G = g1 - g0
            D = int(np.count_nonzero(self.dt_order[f] >= 0))
            rec = {"dt_order": self.dt_order[f, :D].copy(), "dt_scores": np.asarray(scores[f], np.float64)[:D].copy(),
                   "dt_match": self.dt_match[f, :, :, :D].copy(), "dt_ignore": self.dt_ignore[f, :, :, :D].copy(),
                   "gt_match": self.gt_match[A * T * g0:A * T * g1].reshape(A, T, G).copy(),
                   "gt_ignore": self.gt_ig[A * g0:A * g1].reshape(A, G).copy()}
            if self.want_oks:
                rec["oks"] = self.oks[M * g0:M * g0 + D * G].reshape(D, G).copy()
            out.append(rec)
        return out


def keypoint_match(dets, gts, device=0, max_dets=None, thrs=None, area_rng=None, sigmas=None, want_oks=True):
    """COCO keypoint matching of a batch of images on the device (op_keypoint_match), bit-identical
    to keypoint_eval.match_np per image: ``dets`` per image (kpts (D, 17, 3), scores (D,)), ``gts``
    per image ``keypoint_eval.gt_tables``' tuple -> the list of per-image records (match_np's dict;
    ``oks`` only when asked for).  The constants default to keypoint_eval's."""
    n = len(dets)
    if len(gts) != n:
        raise ValueError("keypoint_match: %d images of detections, %d of ground truths" % (n, len(gts)))
    g = _KeypointCall(gts, max_dets, thrs, area_rng, sigmas, want_oks)
    kp = [np.asarray(k, np.float64).reshape(-1, 17, 3) for k, _ in dets]
    sc = [np.asarray(s, np.float64).reshape(-1) for _, s in dets]
    for i in range(n):
        if len(kp[i]) != len(sc[i]):
            raise ValueError("keypoint_match: image %d: %d detections, %d scores" % (i, len(kp[i]), len(sc[i])))
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in sc])
    D = int(off[-1])
    kpts = np.zeros((max(D, 1), 17, 3), np.float64)
    scores = np.zeros(max(D, 1), np.float64)
    if D:
        kpts[:D] = np.concatenate(kp)
        scores[:D] = np.concatenate(sc)
    g.outputs(n)
    if n:
        check(lib().op_keypoint_match(int(device), n, ptr(off), ptr(kpts), ptr(scores), *(
            g.gt_args() + g.const_args() + g.out_args())), "op_keypoint_match")
    return g.records(n, [sc[f][g.dt_order[f][g.dt_order[f] >= 0]] for f in range(n)])


def keypoint_last_ms(device=0):
    """Device time (uploads + kernel, stream events) of the last ``keypoint_match`` /
    ``Context.keypoint_match`` that completed on this device."""
    ms = ctypes.c_double()
    check(lib().op_keypoint_last_ms(int(device), ctypes.byref(ms)), "op_keypoint_last_ms")
    return ms.value


def cpm_layer_table(arch):
    """[(name, ci, co, k)] of FaceNet / HandNet (models/FaceNet.py:11-76) from the library."""
    a = ARCH[arch]
    out = []
    name = ctypes.c_char_p()
    ci, co, k = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    for i in range(lib().op_cpm_layer_count(a)):
        check(lib().op_cpm_layer_info(a, i, ctypes.byref(name), ctypes.byref(ci), ctypes.byref(co), ctypes.byref(k)))
        out.append((name.value.decode(), ci.value, co.value, k.value))
    return out


def cpm_probe_table(arch):
    """[(name, channels, divisor)] of op_cpm_forward_probe's points 0 .. 45 for FaceNet / HandNet, from
    the library: the point's tensor is (frames, channels, h / divisor, w / divisor)."""
    a = ARCH[arch]
    out = []
    name = ctypes.c_char_p()
    ch, div = ctypes.c_int32(), ctypes.c_int32()
    for i in range(N_PROBE_POINTS):
        check(lib().op_cpm_probe_info(a, i, ctypes.byref(name), ctypes.byref(ch), ctypes.byref(div)),
              "op_cpm_probe_info")
        out.append((name.value.decode(), ch.value, div.value))
    return out


def _row_strided_u8(img):
    """A uint8 H x W x 3 view whose pixels are packed within each row (rows may be strided, e.g. a
    crop view into a larger image: the device upload packs them); anything else is copied."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < a.shape[1] * 3:
        a = np.ascontiguousarray(a, np.uint8)
    return a


class PinnedFrames(object):
    """(n, h, w, 3) uint8 frames in page-locked host memory (op_host_alloc), the source of
    asynchronous uploads (Context.upload_frames)."""

    def __init__(self, n, h, w):
        nbytes = int(n) * int(h) * int(w) * 3
        p = ctypes.c_void_p()
        check(lib().op_host_alloc(nbytes, ctypes.byref(p)), "op_host_alloc")
        self._p = p
        buf = (ctypes.c_uint8 * nbytes).from_address(p.value)
        self.array = np.frombuffer(buf, np.uint8).reshape(int(n), int(h), int(w), 3)

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            self.array = None
            lib().op_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CpmContext(object):
    """Owns one op_cpm_ctx: a FaceNet or HandNet replica on one device (face/hand detectors)."""

    def __init__(self, arch, device=0):
        if arch not in ARCH:
            raise ValueError("arch must be one of %s" % sorted(ARCH))
        self.arch = arch
        self.table = cpm_layer_table(arch)
        self.n_maps = self.table[-1][2]
        h = ctypes.c_void_p()
        check(lib().op_cpm_create(ARCH[arch], int(device), ctypes.byref(h)), "op_cpm_create")
        self.h = h

    def set_batch_invariant(self, enable=True):
        """No split-K on small launches: a crop's keypoints and confidences do not depend on the
        other crops of its batch (include/openpose_hip.h: op_cpm_set_batch_invariant)."""
        check(lib().op_cpm_set_batch_invariant(self.h, int(bool(enable))), "op_cpm_set_batch_invariant")

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            lib().op_cpm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_weights(self, weights):
        """weights: {layer: (W (Co,Ci,k,k), b (Co,))} for every layer of the table."""
        Ws, bs = [], []
        for name, ci, co, k in self.table:
            W, b = weights[name]
            W = np.ascontiguousarray(W, np.float32)
            b = np.ascontiguousarray(b, np.float32)
            if W.shape != (co, ci, k, k) or b.shape != (co,):
                raise ValueError("%s: expected W %s b %s, got %s %s" % (name, (co, ci, k, k), (co,), W.shape, b.shape))
            Ws.append(W)
            bs.append(b)
        self._keep = (Ws, bs)
        Wp = (ctypes.c_void_p * len(Ws))(*[w.ctypes.data for w in Ws])
        bp = (ctypes.c_void_p * len(bs))(*[v.ctypes.data for v in bs])
        check(lib().op_cpm_set_weights(self.h, Wp, bp), "op_cpm_set_weights")

    def forward(self, x):
        x = np.ascontiguousarray(x, np.float32)
        n, _, h, w = x.shape
        out = np.empty((n, self.n_maps, h // 8, w // 8), np.float32)
        check(lib().op_cpm_forward(self.h, ptr(x), n, h, w, ptr(out)), "op_cpm_forward")
        return out

    def forward_probe(self, x, point, frames=None, hi=False):
        """What probe point `point` of the forward wrote (include/openpose_hip.h: op_cpm_forward_probe),
        as dense f32 (frames, channels, h / divisor, w / divisor); frames = (first, count), default all.
        hi: the hi halves of the stored split pairs alone (OP_CPM_PROBE_HI) instead of hi + lo."""
        x = np.ascontiguousarray(x, np.float32)
        n, c, h, w = x.shape
        if c != 3:
            raise ValueError("expected (n, 3, h, w)")
        f0, nf = (0, n) if frames is None else (int(frames[0]), int(frames[1]))
        name, ch, div = ctypes.c_char_p(), ctypes.c_int32(), ctypes.c_int32()
        check(lib().op_cpm_probe_info(ARCH[self.arch], int(point), ctypes.byref(name), ctypes.byref(ch),
                                      ctypes.byref(div)), "op_cpm_probe_info")
        out = np.empty((max(nf, 0), ch.value, h // div.value, w // div.value), np.float32)
        check(lib().op_cpm_forward_probe(self.h, ptr(x), n, h, w, int(point) + (CPM_PROBE_HI if hi else 0), f0, nf,
                                         ptr(out), out.size),
              "op_cpm_forward_probe")
        return out

    @staticmethod
    def _keypoints(kp, found):
        return [[int(k[0]), int(k[1]), np.float32(k[2])] if f else None for k, f in zip(kp, found)]

    def peaks(self, heatmaps, thresh, flip=False):
        hm = np.ascontiguousarray(heatmaps, np.float32)
        c, h, w = hm.shape
        kp = np.zeros((max(c - 1, 0), 3), np.float64)
        found = np.zeros(max(c - 1, 0), np.int32)
        check(lib().op_cpm_peaks(self.h, ptr(hm), c, h, w, float(thresh), int(bool(flip)), ptr(kp), ptr(found)),
              "op_cpm_peaks")
        return self._keypoints(kp, found)

    def detect(self, bgr, thresh, flip_maps=False):
        img = _row_strided_u8(bgr)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("expected an H x W x 3 uint8 BGR image")
        h, w = img.shape[:2]
        kp = np.zeros((self.n_maps - 1, 3), np.float64)
        found = np.zeros(self.n_maps - 1, np.int32)
        check(lib().op_cpm_detect(self.h, ctypes.c_void_p(img.ctypes.data), h, w, img.strides[0], float(thresh),
                                  int(bool(flip_maps)), ptr(kp),
                                  ptr(found)), "op_cpm_detect")
        return self._keypoints(kp, found)

    def detect_batch(self, crops, thresh, flip_maps=None):
        """``detect`` over a list of BGR crops (any sizes) in one batched forward; the keypoints of
        one ``detect`` call per crop (confidences up to f32 re-association)."""
        imgs = [_row_strided_u8(c) for c in crops]
        for img in imgs:
            if img.ndim != 3 or img.shape[2] != 3:
                raise ValueError("expected H x W x 3 uint8 BGR crops")
        n, np_ = len(imgs), self.n_maps - 1
        if n == 0:
            return []
        ptrs = (ctypes.c_void_p * n)(*[img.ctypes.data for img in imgs])
        hs = np.array([img.shape[0] for img in imgs], np.int32)
        ws = np.array([img.shape[1] for img in imgs], np.int32)
        rs = np.array([img.strides[0] for img in imgs], np.int64)
        fl = np.array([int(bool(f)) for f in (flip_maps or [False] * n)], np.int32)
        if len(fl) != n:
            raise ValueError("flip_maps needs one entry per crop")
        kp = np.zeros((n, np_, 3), np.float64)
        found = np.zeros((n, np_), np.int32)
        check(lib().op_cpm_detect_batch(self.h, n, ptrs, ptr(hs), ptr(ws), ptr(rs), float(thresh), ptr(fl), ptr(kp),
                                        ptr(found)), "op_cpm_detect_batch")
        return [self._keypoints(kp[i], found[i]) for i in range(n)]

    ROI_GROUP_LAUNCHES = 4  # kRoiGroupLaunches (csrc/cpm.hip): post-process launches per group

    @staticmethod
    def roi_table_bytes(n_frames, n_rois):
        """Bytes of the device tables one ``detect_rois`` call uploads (include/openpose_hip.h)."""
        return 24 * int(n_frames) + 48 * int(n_rois)

    def detect_rois(self, frames, boxes, thresh, frame_ids=None, mirror=None):
        """``detect_batch`` fed from frames and integer boxes (op_cpm_detect_rois): box i =
        (left, top, right, bottom) of ``frames[frame_ids[i]]`` (default: frame 0), read mirrored in x
        where ``mirror[i]`` (default: none).  The crop (roi_crop_np states it), the mirror, the
        resize, the forward, the upsample and the peaks run on the device; each frame is uploaded
        once.  ``frames``: one H x W x 3 uint8 image or a list of them.  The keypoints of
        ``detect_batch([roi_crop_np(...)], thresh, flip_maps=mirror)``, bit for bit."""
        if isinstance(frames, np.ndarray) and frames.ndim == 3:
            frames = [frames]
        imgs = [_row_strided_u8(f) for f in frames]
        for img in imgs:
            if img.ndim != 3 or img.shape[2] != 3:
                raise ValueError("expected H x W x 3 uint8 BGR frames")
        n, nf, np_ = len(boxes), len(imgs), self.n_maps - 1
        if n == 0:
            return []
        bx = np.ascontiguousarray(np.asarray(boxes, np.int64).reshape(n, 4))
        if np.any(np.abs(bx) > 2 ** 31 - 1):
            raise ValueError("op_cpm_detect_rois: box coordinates must fit int32")
        bx = bx.astype(np.int32)
        fi = np.zeros(n, np.int32) if frame_ids is None else np.ascontiguousarray(frame_ids, np.int32)
        mi = np.zeros(n, np.int32) if mirror is None else np.array([int(bool(m)) for m in mirror], np.int32)
        if len(fi) != n or len(mi) != n:
            raise ValueError("frame_ids and mirror need one entry per box")
        ptrs = (ctypes.c_void_p * max(nf, 1))(*[img.ctypes.data for img in imgs])
        hs = np.array([img.shape[0] for img in imgs], np.int32)
        ws = np.array([img.shape[1] for img in imgs], np.int32)
        rs = np.array([img.strides[0] for img in imgs], np.int64)
        kp = np.zeros((n, np_, 3), np.float64)
        found = np.zeros((n, np_), np.int32)
        check(lib().op_cpm_detect_rois(self.h, nf, ptrs, ptr(hs), ptr(ws), ptr(rs), n, ptr(fi), ptr(bx), ptr(mi),
                                       float(thresh), ptr(kp), ptr(found)), "op_cpm_detect_rois")
        return [self._keypoints(kp[i], found[i]) for i in range(n)]

    def detect_rois_staged(self, ctx, first, n_frames, boxes, thresh, frame_ids=None, mirror=None):
        """``detect_rois`` on staged frames [first, first + n_frames) of the ``Context`` ``ctx``, read
        where they lie on the device (op_cpm_detect_rois_staged): box i belongs to staged frame
        ``first + frame_ids[i]`` (default: 0).  Only the tables are uploaded; the ROIs run in chunks
        of ``set_roi_batch``.  The keypoints of ``detect_rois`` on the same frames, bit for bit."""
        n, np_ = len(boxes), self.n_maps - 1
        if n == 0:
            return []
        bx = np.ascontiguousarray(np.asarray(boxes, np.int64).reshape(n, 4))
        if np.any(np.abs(bx) > 2 ** 31 - 1):
            raise ValueError("op_cpm_detect_rois_staged: box coordinates must fit int32")
        bx = bx.astype(np.int32)
        fi = np.zeros(n, np.int32) if frame_ids is None else np.ascontiguousarray(frame_ids, np.int32)
        mi = np.zeros(n, np.int32) if mirror is None else np.array([int(bool(m)) for m in mirror], np.int32)
        if len(fi) != n or len(mi) != n:
            raise ValueError("frame_ids and mirror need one entry per box")
        kp = np.zeros((n, np_, 3), np.float64)
        found = np.zeros((n, np_), np.int32)
        check(lib().op_cpm_detect_rois_staged(self.h, ctx.h, int(first), int(n_frames), n, ptr(fi), ptr(bx), ptr(mi),
                                              float(thresh), ptr(kp), ptr(found)), "op_cpm_detect_rois_staged")
        return [self._keypoints(kp[i], found[i]) for i in range(n)]

    def set_roi_batch(self, rois=0):
        """At most ``rois`` ROIs per forward in ``detect_rois_staged`` (0, the default: all in one)."""
        check(lib().op_cpm_set_roi_batch(self.h, int(rois)), "op_cpm_set_roi_batch")

    def set_roi_group_bytes(self, nbytes=0):
        """Scratch budget of one post-process group of ``detect_rois`` (0: the default)."""
        check(lib().op_cpm_set_roi_group_bytes(self.h, int(nbytes)), "op_cpm_set_roi_group_bytes")

    def roi_stats(self):
        """The last ``detect_rois``: {groups, launches (outside the forward), upload_bytes, scratch_bytes}."""
        out = np.zeros(4, np.int64)
        check(lib().op_cpm_roi_stats(self.h, ptr(out)), "op_cpm_roi_stats")
        return dict(zip(("groups", "launches", "upload_bytes", "scratch_bytes"), (int(v) for v in out)))


class TrainContext(object):
    """Owns one op_train_ctx: CocoPoseNet master weights, Adam state and the activations of a batch
    of n frames of h x w on one device (train_coco_pose_estimation.py's Updater on the GPU)."""

    def __init__(self, n, h, w, device=0):
        self.n, self.h, self.w = int(n), int(h), int(w)
        self.table = layer_table()
        hdl = ctypes.c_void_p()
        check(lib().op_train_create(int(device), self.n, self.h, self.w, ctypes.byref(hdl)), "op_train_create")
        self.h_ = hdl

    def close(self):
        if getattr(self, "h_", None) is not None and self.h_.value:
            lib().op_train_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_weights(self, weights):
        Ws, bs = [], []
        for name, ci, co, k in self.table:
            W, b = weights[name]
            W = np.ascontiguousarray(W, np.float32)
            b = np.ascontiguousarray(b, np.float32)
            if W.shape != (co, ci, k, k) or b.shape != (co,):
                raise ValueError("%s: expected W %s, got %s" % (name, (co, ci, k, k), W.shape))
            Ws.append(W)
            bs.append(b)
        Wp = (ctypes.c_void_p * len(Ws))(*[a.ctypes.data for a in Ws])
        bp = (ctypes.c_void_p * len(bs))(*[a.ctypes.data for a in bs])
        check(lib().op_train_set_weights(self.h_, Wp, bp), "op_train_set_weights")

    def get(self, grads=False):
        """{layer: (W, b)} of the current weights, or of the last step's (unscaled) gradients."""
        out = {name: (np.empty((co, ci, k, k), np.float32), np.empty(co, np.float32))
               for name, ci, co, k in self.table}
        Wp = (ctypes.c_void_p * len(self.table))(*[out[t[0]][0].ctypes.data for t in self.table])
        bp = (ctypes.c_void_p * len(self.table))(*[out[t[0]][1].ctypes.data for t in self.table])
        args = (None, None, Wp, bp) if grads else (Wp, bp, None, None)
        check(lib().op_train_get_weights(self.h_, *args), "op_train_get_weights")
        return out

    def set_hyper(self, alpha, beta1=0.9, beta2=0.999, eps=1e-8):
        check(lib().op_train_set_hyper(self.h_, float(alpha), float(beta1), float(beta2), float(eps)),
              "op_train_set_hyper")

    def enable(self, layer_index, on=True):
        check(lib().op_train_enable_layer(self.h_, int(layer_index), int(bool(on))), "op_train_enable_layer")

    def set_grad_scale(self, layer_index, scale):
        check(lib().op_train_set_grad_scale(self.h_, int(layer_index), float(scale)), "op_train_set_grad_scale")

    def step(self, x, pafs_t, heatmaps_t, ignore_mask):
        n, h8, w8 = self.n, self.h // 8, self.w // 8
        x = np.ascontiguousarray(x, np.float32)
        pt = np.ascontiguousarray(pafs_t, np.float32)
        ht = np.ascontiguousarray(heatmaps_t, np.float32)
        ig = np.ascontiguousarray(ignore_mask, np.uint8)
        if x.shape != (n, 3, self.h, self.w) or pt.shape != (n, 38, h8, w8) or ht.shape != (n, 19, h8, w8) \
                or ig.shape != (n, h8, w8):
            raise ValueError("train step: shapes (n,3,h,w) (n,38,h/8,w/8) (n,19,h/8,w/8) (n,h/8,w/8) expected")
        losses = np.zeros(12, np.float64)
        check(lib().op_train_step(self.h_, ptr(x), ptr(pt), ptr(ht), ptr(ig), ptr(losses)), "op_train_step")
        return losses

    def step_poses(self, x, poses_per_frame, mask=None, heatmap_sigma=7, paf_width=8):
        """``step`` with the targets generated on the device from keypoints (op_train_step_poses):
        poses_per_frame = n arrays (people, 18, 3) of (x, y, visibility) at the network input size,
        mask (n, h, w) nonzero = ignored, or None."""
        x = np.ascontiguousarray(x, np.float32)
        if x.shape != (self.n, 3, self.h, self.w):
            raise ValueError("train step: x (n,3,h,w) expected")
        poses, offsets = pack_poses(poses_per_frame, self.n)
        mk = pack_mask(mask, self.n, self.h, self.w)
        losses = np.zeros(12, np.float64)
        check(lib().op_train_step_poses(self.h_, ptr(x), ptr(poses), ptr(offsets), ptr(mk), float(heatmap_sigma),
                                        float(paf_width), ptr(losses)), "op_train_step_poses")
        return losses

    def last_label_ms(self):
        """Device time of the label part (uploads + kernel) of the last ``step_poses``."""
        ms = ctypes.c_double()
        check(lib().op_train_last_label_ms(self.h_, ctypes.byref(ms)), "op_train_last_label_ms")
        return ms.value

    def _eval_frames(self, x):
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 4 or x.shape[1:] != (3, self.h, self.w) or x.shape[0] < 1:
            raise ValueError("train eval: x (m,3,h,w) with m >= 1 expected")
        if x.shape[0] > self.n:
            raise ValueError("train eval: %d frames, the context holds %d" % (x.shape[0], self.n))
        return x, x.shape[0]

    def eval(self, x, pafs_t, heatmaps_t, ignore_mask):
        """The twelve losses ``step`` would report for these m <= n frames (op_train_eval): forward
        and compute_loss only, nothing of the training state changes."""
        x, m = self._eval_frames(x)
        h8, w8 = self.h // 8, self.w // 8
        pt = np.ascontiguousarray(pafs_t, np.float32)
        ht = np.ascontiguousarray(heatmaps_t, np.float32)
        ig = np.ascontiguousarray(ignore_mask, np.uint8)
        if pt.shape != (m, 38, h8, w8) or ht.shape != (m, 19, h8, w8) or ig.shape != (m, h8, w8):
            raise ValueError("train eval: shapes (m,3,h,w) (m,38,h/8,w/8) (m,19,h/8,w/8) (m,h/8,w/8) expected")
        losses = np.zeros(12, np.float64)
        check(lib().op_train_eval(self.h_, m, ptr(x), ptr(pt), ptr(ht), ptr(ig), ptr(losses)), "op_train_eval")
        return losses

    def eval_poses(self, x, poses_per_frame, mask=None, heatmap_sigma=7, paf_width=8):
        """``eval`` with the targets generated on the device from keypoints (op_train_eval_poses),
        arguments as for ``step_poses`` with m <= n frames."""
        x, m = self._eval_frames(x)
        poses, offsets = pack_poses(poses_per_frame, m)
        mk = pack_mask(mask, m, self.h, self.w)
        losses = np.zeros(12, np.float64)
        check(lib().op_train_eval_poses(self.h_, m, ptr(x), ptr(poses), ptr(offsets), ptr(mk), float(heatmap_sigma),
                                        float(paf_width), ptr(losses)), "op_train_eval_poses")
        return losses

    def get_state(self):
        """{layer: dict(mW, vW, mb, vb, t)}: Adam's moments of W and b and the layer's step count."""
        out = {name: dict(mW=np.empty((co, ci, k, k), np.float32), vW=np.empty((co, ci, k, k), np.float32),
                          mb=np.empty(co, np.float32), vb=np.empty(co, np.float32))
               for name, ci, co, k in self.table}
        ps = [(ctypes.c_void_p * len(self.table))(*[out[t[0]][key].ctypes.data for t in self.table])
              for key in ("mW", "vW", "mb", "vb")]
        t = np.zeros(len(self.table), np.int64)
        check(lib().op_train_get_state(self.h_, ps[0], ps[1], ps[2], ps[3], ptr(t)), "op_train_get_state")
        for i, row in enumerate(self.table):
            out[row[0]]["t"] = int(t[i])
        return out

    def set_state(self, state):
        """Restore what ``get_state`` returned; after ``set_weights``, which zeroes the state."""
        arrs = {key: [] for key in ("mW", "vW", "mb", "vb")}
        for name, ci, co, k in self.table:
            for key, shape in (("mW", (co, ci, k, k)), ("vW", (co, ci, k, k)), ("mb", (co,)), ("vb", (co,))):
                a = np.ascontiguousarray(state[name][key], np.float32)
                if a.shape != shape:
                    raise ValueError("%s/%s: expected %s, got %s" % (name, key, shape, a.shape))
                arrs[key].append(a)
        t = np.ascontiguousarray([int(state[row[0]]["t"]) for row in self.table], np.int64)
        ps = [(ctypes.c_void_p * len(self.table))(*[a.ctypes.data for a in arrs[key]])
              for key in ("mW", "vW", "mb", "vb")]
        check(lib().op_train_set_state(self.h_, ps[0], ps[1], ps[2], ps[3], ptr(t)), "op_train_set_state")

    def buffers(self):
        """[(name, channels, divisor)] of the step's activation buffers (``train_buffer_table``)."""
        return train_buffer_table()

    def read(self, i, grad=False):
        """Activation (or gradient) buffer i as the last step left it (op_train_read_buffer, a test
        aid): (n, channels, h / divisor, w / divisor) f32."""
        _, ch, div = self.buffers()[int(i)]
        out = np.empty((self.n, ch, self.h // div, self.w // div), np.float32)
        check(lib().op_train_read_buffer(self.h_, int(i), int(bool(grad)), ptr(out), out.size), "op_train_read_buffer")
        return out


def pack_poses(poses_per_frame, n=None):
    """n arrays (people, 18, 3) -> (poses (sum, 18, 3) f64, pose_offsets (n + 1,) i32) of op_make_labels."""
    frames = [np.asarray(p, np.float64).reshape(-1, N_JOINTS, 3) for p in poses_per_frame]
    if n is not None and len(frames) != n:
        raise ValueError("expected the poses of %d frames, got %d" % (n, len(frames)))
    offsets = np.zeros(len(frames) + 1, np.int32)
    offsets[1:] = np.cumsum([len(p) for p in frames])
    poses = np.ascontiguousarray(np.concatenate(frames)) if frames else np.zeros((0, N_JOINTS, 3))
    return (poses if len(poses) else None), offsets


def pack_mask(mask, n, h, w):
    """None, or the (n, h, w) u8 ignore mask (nonzero = ignored) of op_make_labels."""
    if mask is None:
        return None
    mk = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    if mk.shape != (n, h, w):
        raise ValueError("ignore mask: %s expected, got %s" % ((n, h, w), mk.shape))
    return mk


def pack_annotations(images):
    """images = n of (h, w, annotations as COCO.loadAnns returns them) -> the flat arrays of
    op_ignore_masks (a dict keyed by its argument names).  The roles follow gen_masks
    (gen_ignore_mask.py:28-36) with labels.train_params' thresholds; a segmentation outside the
    declared limits raises ValueError naming the annotation (masks.segmentation_parts)."""
    from . import masks as _masks
    hw, ann_offsets, role, part_offsets, kind, data_offsets = [], [0], [], [0], [], [0]
    xy, counts = [], []
    for h, w, anns in images:
        hw += [int(h), int(w)]
        for ann in anns:
            role.append(_masks.ann_role(ann))
            for k, data in _masks.segmentation_parts(ann, int(h), int(w)):
                kind.append(k)
                data_offsets.append(data_offsets[-1] + len(data))
                # one index space for both arrays: the other kind's slots are never read
                xy.append(data if k == _masks.KIND_POLYGON else np.zeros(len(data)))
                counts.append(data if k == _masks.KIND_RLE else np.zeros(len(data), np.uint32))
            part_offsets.append(len(kind))
        ann_offsets.append(len(role))
    return dict(hw=np.array(hw, np.int32), ann_offsets=np.array(ann_offsets, np.int32), ann_role=np.array(role, np.int32),
                part_offsets=np.array(part_offsets, np.int32), part_kind=np.array(kind, np.int32),
                data_offsets=np.array(data_offsets, np.int64),
                xy=np.ascontiguousarray(np.concatenate(xy), np.float64) if xy else np.zeros(0, np.float64),
                counts=np.ascontiguousarray(np.concatenate(counts), np.uint32) if counts else np.zeros(0, np.uint32))


def ignore_masks_call(device, n, packed, out_all=None, out_miss=None, out_ann=None):
    """op_ignore_masks on ``pack_annotations``' arrays; out_* are lists of C-contiguous (h, w) u8
    arrays (or None entries, or None) that the call fills."""
    def table(arrays):
        if arrays is None:
            return None
        for a in arrays:
            if a is not None and not (a.dtype == np.uint8 and a.flags.c_contiguous):
                raise ValueError("op_ignore_masks: outputs are C-contiguous uint8 arrays")
        return (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data if a is not None else None for a in arrays])

    def arr(name):
        return ptr(packed[name]) if packed[name].size else None

    tabs = [table(out_all), table(out_miss), table(out_ann)]
    check(lib().op_ignore_masks(int(device), int(n), ptr(packed["hw"]), ptr(packed["ann_offsets"]), arr("ann_role"),
                                ptr(packed["part_offsets"]), arr("part_kind"), ptr(packed["data_offsets"]),
                                arr("xy"), arr("counts"), *tabs), "op_ignore_masks")


def annotation_views_call(device, frames, packed, out_ann=None, out_miss=None):
    """op_annotation_views on ``maskview.pack_views``' arrays: frames are (h, w, 3) uint8 arrays whose
    pixels are packed within a row (packed["row_stride"] bytes per row); out_* are lists of
    C-contiguous (h, w, 3) u8 arrays (or None entries, or None) that the call fills."""
    def table(arrays):
        if arrays is None:
            return None
        for a in arrays:
            if a is not None and not (a.dtype == np.uint8 and a.flags.c_contiguous):
                raise ValueError("op_annotation_views: outputs are C-contiguous uint8 arrays")
        return (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data if a is not None else None for a in arrays])

    def arr(name):
        return ptr(packed[name]) if packed[name].size else None

    n = len(frames)
    bgr = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in frames])
    check(lib().op_annotation_views(int(device), n, bgr, ptr(packed["row_stride"]), ptr(packed["hw"]),
                                    ptr(packed["ann_offsets"]), arr("ann_role"), arr("ann_tint"),
                                    ptr(packed["part_offsets"]), arr("part_kind"), ptr(packed["data_offsets"]),
                                    arr("xy"), arr("counts"), ptr(packed["kp_offsets"]), arr("kp"),
                                    table(out_ann), table(out_miss)), "op_annotation_views")
