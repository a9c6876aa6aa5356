"""ctypes binding of the device C ABI (include/klt_hip.h) of libklt_amd.so.

Used by bench.py and the GPU tests for device-resident work (frames and
feature arrays kept in HBM); the klt.h API (abi.py) is the drop-in surface.
"""
from __future__ import annotations

import ctypes
import ctypes as C
import os

MAX_TAPS = 71
MAX_LEVELS = 8
EXACT, FAST = 0, 1
FB_REJECTED = -6  # KLT_HIP_FB_REJECTED: lost to the forward-backward check (klt_hip_set_fb)
MAX_SEQUENCES = 64  # KLT_HIP_MAX_SEQUENCES: klt_hip_track_frames_multi's nseq
# KLT_HIP_FRAME_*: the pixels of device frames (klt_hip_set_frame_format)
FRAME_GRAY8, FRAME_RGB8, FRAME_BGR8, FRAME_RGBA8, FRAME_BGRA8 = range(5)


class Taps(C.Structure):
    _fields_ = [("width", C.c_int), ("k", C.c_float * MAX_TAPS)]


class PyrDesc(C.Structure):
    _fields_ = [("ncols", C.c_int), ("nrows", C.c_int), ("nlevels", C.c_int),
                ("subsampling", C.c_int), ("smooth_input", C.c_int), ("smooth", Taps),
                ("pyr", Taps), ("grad_gauss", Taps), ("grad_deriv", Taps)]


class TrackDesc(C.Structure):
    _fields_ = [("window_width", C.c_int), ("window_height", C.c_int),
                ("max_iterations", C.c_int), ("min_determinant", C.c_float),
                ("min_displacement", C.c_float), ("max_residue", C.c_float),
                ("step_factor", C.c_float), ("borderx", C.c_int), ("bordery", C.c_int),
                ("lighting_insensitive", C.c_int), ("reduction", C.c_int)]


class AffineDesc(C.Structure):
    """klt_hip_affine_desc: the affine consistency check's parameters."""
    _fields_ = [("mode", C.c_int), ("window_width", C.c_int), ("window_height", C.c_int),
                ("max_iterations", C.c_int), ("min_determinant", C.c_float),
                ("min_displacement", C.c_float), ("affine_min_displacement", C.c_float),
                ("max_residue", C.c_float), ("max_displacement_differ", C.c_float),
                ("step_factor", C.c_float), ("lighting_insensitive", C.c_int)]

    @classmethod
    def from_tc(cls, tc) -> "AffineDesc":
        """What KLTTrackFeatures passes for this tracking context (a TrackingContextRec)."""
        return cls(tc.affineConsistencyCheck, tc.affine_window_width, tc.affine_window_height,
                   tc.affine_max_iterations, tc.min_determinant, tc.min_displacement,
                   tc.affine_min_displacement, tc.affine_max_residue, tc.affine_max_displacement_differ,
                   tc.step_factor, tc.lighting_insensitive)


class SelectDesc(C.Structure):
    _fields_ = [("window_width", C.c_int), ("window_height", C.c_int), ("borderx", C.c_int),
                ("bordery", C.c_int), ("nSkippedPixels", C.c_int)]


class ReplaceDesc(C.Structure):
    """klt_hip_replace_desc: replacement of lost features inside the batched calls."""
    _fields_ = [("sel", SelectDesc), ("mindist", C.c_int), ("min_eigenvalue", C.c_int), ("every", C.c_int)]

    @classmethod
    def from_tc(cls, tc, every: int) -> "ReplaceDesc":
        """What KLTTrackSequenceReplace passes for this tracking context (a TrackingContextRec)."""
        sel = SelectDesc(tc.window_width, tc.window_height, max(tc.borderx, tc.window_width // 2),
                         max(tc.bordery, tc.window_height // 2), tc.nSkippedPixels)
        return cls(sel, tc.mindist, tc.min_eigenvalue, every)


class Timing(C.Structure):
    _fields_ = [("n_pyr_l0", C.c_int), ("n_pyr_l1", C.c_int), ("n_track", C.c_int),
                ("n_eigen", C.c_int), ("n_generic", C.c_int), ("ms_pyr_l0", C.c_double),
                ("ms_pyr_l1", C.c_double), ("ms_track", C.c_double), ("ms_eigen", C.c_double),
                ("ms_generic", C.c_double), ("frames_pyr_l0", C.c_long), ("frames_pyr_l1", C.c_long),
                ("frames_track", C.c_long)]


V = C.c_void_p
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
DP = C.POINTER(C.c_double)

DEVICE_PROTOS = {
    "klt_hip_ctx_create": (V, [C.c_int]),
    "klt_hip_ctx_destroy": (None, [V]),
    "klt_hip_last_error": (C.c_char_p, [V]),
    "klt_hip_track_kernel": (C.c_char_p, [V]),
    "klt_hip_set_stream": (C.c_int, [V, V]),
    "klt_hip_get_stream": (V, [V]),
    "klt_hip_sync": (C.c_int, [V]),
    "klt_hip_device_count": (C.c_int, []),
    "klt_hip_current_device": (C.c_int, []),
    "klt_hip_upload_frame": (C.c_int, [V, C.c_int, V, C.c_int, C.c_int]),
    "klt_hip_build_pyramid": (C.c_int, [V, C.c_int, C.POINTER(PyrDesc), V, C.c_long, C.c_int]),
    "klt_hip_frame_bpp": (C.c_int, [C.c_int]),
    "klt_hip_set_frame_format": (C.c_int, [V, C.c_int]),
    "klt_hip_get_frame_format": (C.c_int, [V]),
    "klt_hip_gray_host": (C.c_int, [C.c_int, V, C.c_long, C.c_int, C.c_int, V, C.c_long]),
    "klt_hip_to_gray": (C.c_int, [V, C.c_int, V, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, V, C.c_long,
                                  C.c_long]),
    "klt_hip_pyramid_path": (C.c_int, [V, C.c_int]),
    "klt_hip_fused_path": (C.c_int, [V, C.POINTER(PyrDesc)]),
    "klt_hip_set_track_order": (C.c_int, [V, C.c_int]),
    "klt_hip_set_track_merge": (C.c_int, [V, C.c_int]),
    "klt_hip_set_lazy_grad": (C.c_int, [V, C.c_int]),
    "klt_hip_set_l0_strip": (C.c_int, [V, C.c_int]),
    "klt_hip_set_track_prio": (C.c_int, [V, C.c_int]),
    "klt_hip_set_track_impl": (C.c_int, [V, C.c_int]),
    "klt_hip_set_track_patch": (C.c_int, [V, C.c_int]),
    "klt_hip_set_fb": (C.c_int, [V, C.c_int, C.c_float]),
    "klt_hip_get_fb": (C.c_int, [V, IP, FP]),
    "klt_hip_set_fb_table": (C.c_int, [V, V, C.c_long]),
    "klt_hip_set_predict": (C.c_int, [V, C.c_int, V, V]),
    "klt_hip_get_predict": (C.c_int, [V, IP, C.POINTER(V), C.POINTER(V)]),
    "klt_hip_set_predict_table": (C.c_int, [V, V, V, C.c_long]),
    # dev_mask, pitch, flags (MASK_SELECT | MASK_TRACK)
    "klt_hip_set_mask": (C.c_int, [V, V, C.c_long, C.c_int]),
    "klt_hip_get_mask": (C.c_int, [V, C.POINTER(V), C.POINTER(C.c_long), IP]),
    "klt_hip_set_frames_affine": (C.c_int, [V, C.POINTER(AffineDesc), V, V]),
    "klt_hip_get_frames_affine": (C.c_int, [V, IP]),
    "klt_hip_set_affine_table": (C.c_int, [V, V, V, C.c_long]),
    "klt_hip_affine_state_put": (C.c_int, [V, FP, IP, C.c_int, C.POINTER(V), C.POINTER(V)]),
    "klt_hip_affine_state_get": (C.c_int, [V, FP, IP, C.c_int]),
    "klt_hip_affine_reserve": (C.c_int, [V, C.c_int, C.c_int, C.c_int]),
    "klt_hip_affine_put": (C.c_int, [V, IP, C.c_int, FP]),
    "klt_hip_affine_get": (C.c_int, [V, IP, C.c_int, FP]),
    "klt_hip_track_affine": (C.c_int, [V, C.c_int, C.c_int, C.POINTER(TrackDesc), C.POINTER(AffineDesc), FP, FP, IP,
                                       FP, IP, C.c_int]),
    "klt_hip_set_frames_replace": (C.c_int, [V, C.POINTER(ReplaceDesc)]),
    "klt_hip_get_frames_replace": (C.c_int, [V, IP, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "klt_hip_frames_replace_changed": (C.c_int, [V, V, C.c_int]),
    "klt_hip_min_eigen_plane": (C.c_int, [V, V, C.c_int, C.c_int, C.POINTER(SelectDesc), V]),
    "klt_hip_eigen_kernel": (C.c_char_p, [V]),
    "klt_hip_set_track_count": (C.c_int, [V, C.c_int]),
    "klt_hip_get_track_count": (C.c_int, [V, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.c_int]),
    "klt_hip_set_prof": (C.c_int, [V, V]),
    "klt_hip_set_frames_overlap": (C.c_int, [V, C.c_int]),
    "klt_hip_set_frames_tail": (C.c_int, [V, C.c_int]),
    "klt_hip_tail_threshold": (C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_uint)]),
    "klt_hip_set_wave_times": (C.c_int, [V, V]),
    "klt_hip_order_slot": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, IP]),
    "klt_hip_band_order_probe": (C.c_int, [V, V, V, C.c_int, C.c_int, V]),
    "klt_hip_set_host_threads": (C.c_int, [V, C.c_int]),
    "klt_hip_get_host_threads": (C.c_int, [V]),
    "klt_hip_set_path": (C.c_int, [V, C.c_int]),
    "klt_hip_set_bank_budget": (C.c_int, [V, C.c_size_t]),
    "klt_hip_get_bank_budget": (C.c_size_t, [V]),
    "klt_hip_frames_chunk": (C.c_int, [V]),
    "klt_hip_ctx_footprint": (C.c_size_t, [V]),
    "klt_hip_ctx_reset": (C.c_int, [V]),
    "klt_hip_level_dims": (C.c_int, [V, C.c_int, C.c_int, IP, IP]),
    "klt_hip_download_level": (C.c_int, [V, C.c_int, C.c_int, C.c_int, V]),
    "klt_hip_level_ptr": (V, [V, C.c_int, C.c_int, C.c_int]),
    "klt_hip_level_interleaved": (C.c_int, [V, C.c_int, C.c_int]),
    "klt_hip_track": (C.c_int, [V, C.c_int, C.c_int, C.POINTER(TrackDesc), V, V, V, C.c_int, C.c_int]),
    "klt_hip_track_sequence": (C.c_int, [V, C.POINTER(PyrDesc), C.POINTER(TrackDesc), V, C.c_long,
                                         C.c_long, C.c_int, C.c_int, V, V, V, C.c_int, IP]),
    "klt_hip_frames_begin": (C.c_int, [V, C.POINTER(PyrDesc), V, C.c_long]),
    "klt_hip_frames_begin_slot": (C.c_int, [V, C.c_int]),
    "klt_hip_frames_end_slot": (C.c_int, [V, C.c_int]),
    "klt_hip_track_frames": (C.c_int, [V, C.POINTER(PyrDesc), C.POINTER(TrackDesc), V, C.c_long, C.c_long,
                                       C.c_int, C.c_int, V, V, V, C.c_int, V, V, V, C.c_long]),
    # n_seq: host int[nseq]
    "klt_hip_track_frames_multi": (C.c_int, [V, C.POINTER(PyrDesc), C.POINTER(TrackDesc), V, C.c_long, C.c_long,
                                             C.c_long, C.c_int, C.c_int, C.c_int, IP, V, V, V, V, V, V, C.c_long]),
    "klt_hip_multi_covers": (C.c_int, [V, C.POINTER(PyrDesc), C.POINTER(TrackDesc)]),
    # rep, count0, then klt_hip_track_frames_multi's, then host changed (n bytes), runs and filled (long[nseq])
    "klt_hip_track_frames_multi_replace": (C.c_int, [V, C.POINTER(PyrDesc), C.POINTER(TrackDesc),
                                                     C.POINTER(ReplaceDesc), C.c_long, V, C.c_long, C.c_long,
                                                     C.c_long, C.c_int, C.c_int, C.c_int, IP, V, V, V, V, V, V,
                                                     C.c_long, V, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    # dev_rec, frame_stride (floats), which (host int[nsel]), nsel, ncols, nrows, desc, dev_maps
    "klt_hip_min_eigen_records": (C.c_int, [V, V, C.c_long, IP, C.c_int, C.c_int, C.c_int, C.POINTER(SelectDesc), V]),
    # frames: const unsigned char *const *; rows: klt_hip_rows_fn or NULL
    "klt_hip_track_frames_host": (C.c_int, [V, C.POINTER(PyrDesc), C.POINTER(TrackDesc), V, C.c_int, C.c_int,
                                            C.c_int, V, V, V, C.c_int, V, V]),
    "klt_hip_track_frames_band": (C.c_int, [V, C.POINTER(PyrDesc), C.POINTER(TrackDesc), V, C.c_long, C.c_long,
                                            C.c_int, V, V, V, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, V,
                                            V, C.c_int]),
    "klt_shard_unique_id": (C.c_int, [V]),
    "klt_shard_band_edges": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "klt_shard_create": (V, [V, C.c_int, C.c_int, V, C.c_int, C.c_int]),
    "klt_shard_create_local": (V, [V, C.c_int, C.c_int, C.c_int, C.c_int]),
    "klt_shard_destroy": (None, [V]),
    "klt_shard_last_error": (C.c_char_p, [V]),
    "klt_shard_create_error": (C.c_char_p, []),
    "klt_shard_inject_fault": (C.c_int, [V, C.c_int]),
    "klt_shard_rows": (C.c_int, [V, IP, IP]),
    "klt_shard_track": (C.c_int, [V, C.POINTER(PyrDesc), C.POINTER(TrackDesc), V, C.c_long, C.c_long, C.c_int, V,
                                  C.c_int, V, V, V, C.c_int, V, V]),
    "klt_hip_select_map": (C.c_int, [V, C.c_int, C.c_int, V, C.c_int, C.c_int, V, V, V, V, C.c_int]),
    "klt_hip_min_eigen_rows": (C.c_int, [V, V, C.c_int, C.c_int, V, IP, IP, IP, IP]),
    "klt_hip_gather_order": (C.c_int, [V, V, V, V, C.c_int, FP, C.c_int, V, V, V, V]),
    "klt_hip_gather_pack": (C.c_int, [V, V, V, V, V, C.c_int, C.c_int, C.c_int, V, C.c_int, V, C.c_int]),
    "klt_hip_gather_unpack": (C.c_int, [V, V, C.c_int, C.c_int, V, C.c_int, C.c_int, C.c_int, V, V, V, V, V]),
    "klt_hip_gather_work_ints": (C.c_long, [C.c_int, C.c_int]),
    "klt_hip_gather_unpack_order": (C.c_int, [V, V, C.c_int, C.c_int, V, C.c_int, C.c_int, C.c_int, V, V, V, V, V,
                                              FP, V, V, V]),
    "klt_hip_set_ahead_ready": (C.c_int, [V, C.c_int]),
    "klt_shard_eigen": (C.c_int, [V, C.POINTER(PyrDesc), V, C.c_long, V, V, V]),
    "klt_shard_select": (C.c_int, [V, C.POINTER(PyrDesc), V, C.c_int, C.c_int, V, V, V, V, C.c_int]),
    "klt_shard_replace": (C.c_int, [V, C.POINTER(PyrDesc), V, C.c_long, C.c_int, C.c_int, V, V, V, C.c_int, V, V]),
    "klt_hip_min_eigen": (C.c_int, [V, C.c_int, C.POINTER(SelectDesc), V, IP, IP]),
    "klt_hip_select": (C.c_int, [V, C.c_int, C.POINTER(SelectDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 V, V, V, V, C.c_int]),
    "klt_hip_select_dev_map": (C.c_int, [V, V, C.c_int, C.c_int, C.POINTER(SelectDesc), C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, V, V, V, V, C.c_int]),
    "klt_hip_select_tune": (C.c_int, [V, C.c_int]),
    "klt_hip_select_stats": (C.c_int, [V, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long), DP]),
    "klt_hip_select_sort_test": (C.c_int, [V, V, C.c_int, V, V]),
    "klt_hip_synth_rows": (C.c_int, [V, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, V,
                                     C.c_long, C.c_long]),
    "klt_hip_synth_frames": (C.c_int, [V, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, V,
                                       C.c_long, C.c_long]),
    "klt_hip_malloc": (V, [V, C.c_size_t]),
    "klt_hip_free": (None, [V, V]),
    "klt_hip_memcpy": (C.c_int, [V, V, V, C.c_size_t, C.c_int]),
    "klt_hip_set_timing": (C.c_int, [V, C.c_int]),
    "klt_hip_get_timing": (C.c_int, [V, C.POINTER(Timing)]),
    "klt_hip_selftest_sqrt": (C.c_int, [V, DP, DP, C.c_int]),
    "klt_hip_selftest_div": (C.c_int, [V, FP, FP, FP, C.c_int]),
    "klt_hip_selftest_solve2": (C.c_int, [V, FP, C.c_float, C.c_float, FP, C.POINTER(C.c_int), C.c_int]),
    "klt_hip_selftest_copy_pool": (C.c_int, [C.c_int, C.c_int, C.c_size_t]),
    # klt_api.c hooks
    "klt_amd_device_context": (V, [V]),
    "klt_amd_pyr_desc": (None, [V, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PyrDesc)]),
    "klt_amd_track_desc": (None, [V, C.POINTER(TrackDesc)]),
    "klt_amd_set_reduction": (None, [V, C.c_int]),
    "klt_amd_set_fb_check": (C.c_int, [V, C.c_int, C.c_float]),
    "klt_amd_set_prediction": (C.c_int, [V, C.c_int]),
    # host_mask (ncols x nrows bytes), ncols, nrows, flags
    "klt_amd_set_mask": (C.c_int, [V, V, C.c_int, C.c_int, C.c_int]),
    "klt_amd_release_cached_devices": (C.c_int, []),
    "klt_amd_register_buffer": (C.c_int, [V, V, C.c_size_t]),
    "klt_amd_unregister_buffer": (C.c_int, [V, V]),
    "klt_hip_register_host": (C.c_int, [V, V, C.c_size_t]),
    "klt_hip_unregister_host": (C.c_int, [V, V]),
    # host helpers
    "klt_synth_frame": (None, [C.c_uint64, C.c_int, C.c_int, C.c_int, V]),
    "klt_sort_pairs_full": (None, [IP, IP, C.c_int]),
}

H2D, D2H, D2D = 1, 2, 3  # hipMemcpyKind
MASK_SELECT, MASK_TRACK = 1, 2  # klt_hip_set_mask's flags
MASKED = -7  # KLT_HIP_MASKED / KLT_AMD_MASKED


def bind_device(lib: C.CDLL) -> C.CDLL:
    # KLT_AMD_LIB may name an older build (same-box A/B tools): its missing
    # extensions stay unbound; the shipped library exports all of them
    # (tests/test_abi.py)
    alt = bool(os.environ.get("KLT_AMD_LIB"))
    for name, (res, args) in DEVICE_PROTOS.items():
        if alt and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


class DeviceError(RuntimeError):
    pass


def check(lib: C.CDLL, ctx, rc: int, what: str) -> None:
    if rc != 0:
        msg = lib.klt_hip_last_error(ctx)
        raise DeviceError(f"{what}: {msg.decode() if msg else 'error'}")


def use_torch_stream(lib, ctx, device=None):
    """Run the library and torch on one stream.  torch's default stream is the
    null stream (handle 0), which klt_hip_set_stream reads as "the context's
    own non-blocking stream" -- unordered with torch.  So make a dedicated
    torch stream current and hand that to the library.  Returns the stream."""
    import torch
    s = torch.cuda.current_stream(device)
    if s.cuda_stream == 0:
        s = torch.cuda.Stream(device)
        torch.cuda.set_stream(s)
    check(lib, ctx, lib.klt_hip_set_stream(ctx, ctypes.c_void_p(s.cuda_stream)), "set_stream")
    return s
