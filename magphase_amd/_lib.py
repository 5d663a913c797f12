"""
ctypes binding of libmagphase_hip.so (C ABI: include/magphase_hip.h).

There is NO CPU fallback: if the library is missing or no ROCm device is visible the product raises.
"""
import ctypes
import threading
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmagphase_hip.so")

vp, i32, i64, sz, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_double   # (C int is i32)
u32 = ctypes.c_uint32

# every symbol include/magphase_hip.h declares: name -> (restype, argtypes), in the header's order
# (tests/test_cabi_symbols.py checks the header against this table and that the .so exports them all)
PROTOTYPES = {
    "mpx_version": (i32, []),
    "mpx_last_error": (ctypes.c_char_p, []),
    "mpx_tables_bytes": (sz, [i32]),
    "mpx_tables_init": (i32, [vp, i32, vp]),
    "mpx_feat_ld": (i64, [i32]),
    "mpx_analysis_frames": (i32, [vp, i32] + [vp] * 5 + [i64, vp, vp, vp, i64]),
    "mpx_tables_f64_bytes": (sz, [i32]),
    "mpx_tables_f64_init": (i32, [vp, i32, vp]),
    "mpx_analysis_frames_f64": (i32, [vp, i32] + [vp] * 5 + [i64, vp, vp, vp, i64, vp]),
    "mpx_analysis_frames_f64w": (i32, [vp, i32] + [vp] * 5 + [i64, vp, vp, vp, i64, vp, vp, i32]),
    "mpx_analysis_compressed_fused": (i32, [vp, i32] + [vp] * 5 + [i64, vp, i32, vp, vp, i32, i32, vp, i32, vp, vp,
                                       vp]),
    "mpx_analysis_compressed_fused_cr": (i32, [vp, i32] + [vp] * 5 + [i64, vp, i32, vp, vp, i32, i32] + [vp] * 4 +
                                          [i64] + [vp] * 4),
    "mpx_analysis_compressed_fused_cr_work_bytes": (i64, [i32, i64]),
    "mpx_analysis_compressed_fused_tiles": (i32, [i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]),
    "mpx_analysis_compressed_fused_waves": (i32, []),
    "mpx_analysis_compressed_fused_layout": (i32, []),
    "mpx_analysis_compressed_fused_blocks_per_cu": (i32, [i32, i32]),
    "mpx_synthesis_lossless_frames": (i32, [vp, i32] + [vp] * 4 + [i64, vp, i64]),
    "mpx_ola_gather": (i32, [vp, i32, vp, i32] + [vp] * 4 + [i64, vp]),
    "mpx_synth_ola_slots": (i32, []),
    "mpx_synth_ola_slot_weights": (i32, [vp, i32]),
    "mpx_ola_strip_floats": (i64, [i32]),
    "mpx_synthesis_lossless_ola": (i32, [vp, i32] + [vp] * 5 + [i32, vp, vp, i32, vp, vp, vp, i64]),
    "mpx_synthesis_lossless_ola_lerp": (i32, [vp, i32] + [vp] * 8 + [i32, vp, vp, i32, vp, vp, vp, i64]),
    "mpx_rows_lerp": (i32, [vp, i32, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64]),
    "mpx_synthesis_lossless_backward": (i32, [vp, i32, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64] + [vp] * 6 + [i64]),
    "mpx_synthesis_compressed_backward": (i32, [vp, i32, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64] + [vp] * 12
                                          + [i32, vp, vp, vp, i64]),
    "mpx_synthesis_compressed_type2_backward": (i32, [vp, i32, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64] + [vp] * 12
                                                + [i32, vp, vp, vp, i64]),
    "mpx_rows_lerp_adjoint": (i32, [vp, i32, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, i64]),
    "mpx_analysis_lossless_backward": (i32, [vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, i64,
                                             vp, i64]),
    "mpx_analysis_lossless_const_rate_backward": (i32, [vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, i64, i64, vp, vp, vp, vp,
                                                        vp, vp, i64, vp, i64, vp, i64]),
    "mpx_ola_fixup": (i32, [vp, i32, vp, i32, vp, vp]),
    "mpx_ola_fixup_width": (i32, [vp, i32, vp, i32, vp, vp, i32]),
    "mpx_roundtrip_lossless_ola": (i32, [vp, i32] + [vp] * 5 + [i64, vp, i32, vp, vp, i32] + [vp] * 6 + [i64]),
    "mpx_roundtrip_lossless_ola_flags": (i32, [vp, i32] + [vp] * 5 + [i64, vp, i32, vp, vp, i32] + [vp] * 6 + [i64, u32]),
    "mpx_roundtrip_support_classes": (i32, [i32, vp, vp, i64, vp]),
    "mpx_roundtrip_frame_extents": (i32, [i32, vp, vp, i64, u32, vp]),
    "mpx_roundtrip_store_map": (i32, [i32, i32, vp]),
    "mpx_roundtrip_slot_weights": (i32, [vp, i32]),
    "mpx_roundtrip_frame_terms": (i32, [i32, vp, vp, i64, vp]),
    "mpx_roundtrip_slot_costs": (i32, [vp, i32]),
    "mpx_griffin_lim_ola": (i32, [vp, i32] + [vp] * 5 + [i64, vp, vp, i32, vp, vp, i32] + [vp] * 4 + [i64]),
    "mpx_griffin_lim_fold": (i32, [vp, i32, i32, vp, vp, i64, i64, i64, vp, vp, vp, vp, i64]),
    "mpx_mel_unwarp": (i32, [vp, i64, i32, vp, i32] + [vp] * 4 + [i32, vp, vp, vp, i64]),
    "mpx_mel_unwarp_rows": (i32, [vp, i64, i32, vp, i32] + [vp] * 4 + [i32, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp,
                             i32]),
    "mpx_spec_ld": (i64, [i32]),
    "mpx_noise_uniform": (i32, [vp, i32, vp, vp, i64, vp]),
    "mpx_noise_numpy_mt19937": (i32, [vp, vp, i32, i64] + [vp] * 5),
    "mpx_noise_numpy_mt19937_work_words": (i64, []),
    "mpx_host_mt19937_jump_poly": (i32, [i64, i32, vp]),
    "mpx_host_mt19937_jump_polys": (i32, [vp, i32, vp, i32]),
    "mpx_noise_stats": (i32, [vp, i32] + [vp] * 6 + [i64, vp]),
    "mpx_noise_spectra_floats": (i64, [i32, i64]),
    "mpx_noise_stats_spectra": (i32, [vp, i32] + [vp] * 6 + [i64, vp, vp]),
    "mpx_synth_comp_slots": (i32, []),
    "mpx_synth_comp_slot_weights": (i32, [vp, i32]),
    "mpx_synthesis_compressed_ola": (i32, [vp, i32] + [vp] * 21 + [i32, vp, vp, i32, vp, vp, i64, i32]),
    "mpx_synthesis_compressed_type2_ola": (i32, [vp, i32] + [vp] * 21 + [i32, vp, vp, i32, vp, vp, i64, i32]),
    "mpx_synthesis_compressed_ola_spectra": (i32, [vp, i32] + [vp] * 21 + [i32, vp, vp, i32, vp, vp, i64, i32, vp]),
    "mpx_host_const_to_var_scan": (i64, [vp, vp, i64, vp, vp]),
    "mpx_host_const_to_var_scan_cap": (i64, [vp, vp, i64, vp, vp, i64]),
    "mpx_host_plan_analysis": (i64, [i32] + [vp] * 12),
    "mpx_host_plan_analysis_batch": (i64, [i32] + [vp] * 8 + [i32] + [vp] * 9 + [i32, vp, vp, i64, vp, i32]),
    "mpx_host_plan_synthesis": (i64, [i32, vp, vp, f64, i32, i32, i32, i64] + [vp] * 17),
    "mpx_host_plan_synthesis_batch": (i64, [i32] + [vp] * 5 + [i32, i32, vp, vp, f64] + [i32] * 4 + [vp, f64, i32, vp,
                                       i64] + [vp] * 9 + [i64, vp, i32]),
    "mpx_host_plan_lossless_synthesis": (i64, [i32, vp, vp, vp, i32] + [vp] * 4),
    "mpx_host_ola_runs": (i64, [i32] + [vp] * 5 + [i32, vp, i64, vp, i64]),
    "mpx_host_ola_runs_extents": (i64, [i32] + [vp] * 5 + [i32, vp, i64, vp, vp, i64]),
    "mpx_host_deal_cuts": (i64, [vp, i64, i32, vp, i32, vp, vp]),
    "mpx_host_widen_f32": (i32, [vp, vp, i64, i32]),
    "mpx_host_narrow_f64": (i32, [vp, vp, i64, i32]),
    "mpx_host_copy_many": (i32, [i32] + [vp] * 4 + [i32]),
    "mpx_host_file_sizes": (i32, [i32, vp, vp]),
    "mpx_host_read_est_batch": (i32, [i32, vp, i32] + [vp] * 4 + [i32]),
    "mpx_host_write_files": (i32, [i32] + [vp] * 6 + [i32]),
    "mpx_host_read_files": (i32, [i32] + [vp] * 4 + [i32]),
    "mpx_mel_warp": (i32, [vp, i64, i32] + [vp] * 7 + [i32, vp, i32] + [vp] * 4 + [i64]),
    "mpx_mel_warp_fbank": (i32, [vp, i64, i32] + [vp] * 7 + [i32, vp, i32] + [vp] * 4 + [i64]),
    "mpx_mel_warp_rows": (i32, [vp, i64, i32] + [vp] * 7 + [i32, vp, i32] + [vp] * 4 + [i64, i32, i64, vp, vp, vp]),
    "mpx_warp_phase_rows": (i32, [vp, i64, i32] + [vp] * 8),
    "mpx_mel_warp_backward": (i32, [vp, i32, vp, vp, i32, vp, i64] + [vp] * 7 + [i32, vp, vp, i64, vp, vp, vp, i64, i64]),
    "mpx_mel_unwarp_backward": (i32, [vp, i32, vp, i64, vp, i64, vp, i32, i64, vp, vp, vp, i64, i32, vp, i32, i64, vp, vp]),
    "mpx_phase_grad_mask": (i32, [vp, i64, i32] + [vp] * 7),
    "mpx_min_phase": (i32, [vp, i32] + [vp] * 5 + [i64, vp, vp, vp, i64]),
    "mpx_min_phase_backward": (i32, [vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, i64, i32, i64, vp, i64]),
    "mpx_true_envelope": (i32, [vp, i32, vp, vp, vp, i64, i64, i32, f64, i32, vp, i64, vp, vp, vp]),
    "mpx_true_envelope_backward": (i32, [vp, i32, vp, vp, vp, i64, i64, i32, i32, vp, vp, i64, vp, i64, vp, vp, i64, vp]),
    "mpx_frame_gain": (i32, [vp, i32] + [vp] * 5 + [i64, vp, i32]),
    "mpx_noise_gains": (i32, [vp] * 4 + [i32, i32, vp, vp]),
    "mpx_noise_power": (i32, [vp, i32] + [vp] * 5 + [i64, vp]),
    "mpx_noise_rms": (i32, [vp, i32, vp, vp, i32, vp, vp]),
    "mpx_post_filter": (i32, [vp, vp, i64, i32, vp, i32, i32, vp, vp]),
    "mpx_epoch_f0_track": (i32, [vp, vp, vp, i32, i32, vp, i64, vp, vp, vp, i64] + [i32] * 4 + [f64, vp, vp, vp]),
    "mpx_epoch_zff": (i32, [vp, vp, vp, i32, i64, vp, i32, vp, vp, vp, i32] + [vp] * 5),
    "mpx_pcm16": (i32, [vp, vp, i32, vp, i32, i64, f64, vp, vp]),
    "mpx_pcm16_to_f32": (i32, [vp, vp, i64, vp]),
    "mpx_hpf_block": (i32, []),
    "mpx_output_hpf": (i32, [vp] * 4 + [i32, i64] + [vp] * 7),
    "mpx_bw_probe": (i32, [vp, i32, vp, vp, i64]),
    "mpx_bw_probe_shapes": (i32, []),
    "mpx_rows_pack": (i32, [vp, vp, vp, i32, i32] + [vp, i32, i64, i64] * 3),
    "mpx_post_filter_merlin": (i32, [vp, vp, i64, i32] + [vp] * 4 + [i32, f64, vp, f64] + [vp] * 5),
    "mpx_post_filter_backward": (i32, [vp, vp, i64, i32, vp, vp, vp, i32, vp]),
    "mpx_post_filter_merlin_backward": (i32, [vp, vp, vp, i64, i32] + [vp] * 4 + [i32] + [vp] * 7),
    "mpx_mlpg_work_doubles": (i64, [i64, i32]),
    "mpx_mlpg_solve": (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, i64, i32, i32, vp, i32, vp, i64, vp]),
    "mpx_mlpg_apply": (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, i64, i32, i32, vp, vp, i64]),
    "mpx_mlpg_colsum_work_doubles": (i64, [i64, i64]),
    "mpx_mlpg_column_sums": (i32, [vp, vp, i64, i64, i64, vp, vp]),
    "mpx_mlpg_var_backward": (i32, [vp, vp, i64, vp, i64, vp, i32, i64, vp, i32, i64, vp, i32, i64, i32, i32, vp, vp, i64,
                                    vp, vp]),
    "mpx_mlpg_trajectory_nll": (i32, [vp, vp, i64, vp, i32, i64, vp, i32, i64, vp, i32, i64, i32, i32, vp, vp]),
    "mpx_mlpg_nll_work_doubles": (i64, [i64, i32]),
    "mpx_mlpg_trajectory_nll_backward": (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i64, vp, i32, i64, vp, vp, i32, i64,
                                               i32, i32, vp, vp, i64, vp, i64, vp]),
    "mpx_cmp_voiced_neighbours": (i32, [vp, vp, i32, i64, vp, i32, i64, vp]),
    "mpx_cmp_compose": (i32, [vp, vp, i32, i64, vp, i32, i32, i32, f64, i32, vp, vp, i32, i64, i32, vp, vp, vp, vp, i32,
                              i64]),
    "mpx_cmp_compose_backward": (i32, [vp, vp, i64, vp, i32, i32, i32, vp, vp, i32, i64, i32, vp, vp, vp, i64]),
    "mpx_cmp_moments_work_doubles": (i64, [i64, i64]),
    "mpx_cmp_column_moments": (i32, [vp, vp, i32, i64, i64, i64, vp, vp]),
}
SYMBOLS = tuple(PROTOTYPES)
# mpx_roundtrip_lossless_ola_flags: how the feature rows are stored (MPX_RT_STORE_ROWS, by line, MPX_RT_STORE_NT), by the
# names MAGPHASE_RT_STORES takes
RT_STORE_FLAGS = {"rows": 4, "lines": 0, "lines_nt": 8}
# ... and how the waveform is rebuilt at N = 4096 (the windowed frame added directly, or MPX_RT_INVERSE_TRANSFORM), by the
# names MAGPHASE_RT_INVERSE takes
RT_INVERSE_FLAGS = {"direct": 0, "transform": 32}
del vp, i32, i64, sz, f64

_lib = None


class MagphaseHipError(RuntimeError):
    pass


_load_lock = threading.Lock()


def load():
    """Loads the shared library (once) and declares the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    with _load_lock:   # the reader / writer threads of iobatch call the host helpers: one loader at a time
        return _load_locked()


def _load_locked():
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch first: it brings the process's HIP runtime (its own libamdhip64).  Loading this library before it binds
    # the kernels to a second copy of the runtime from /opt/rocm, which torch never initialises ("no ROCm-capable
    # device is detected" at the first launch).
    import torch  # noqa: F401
    if not os.path.isfile(LIB_PATH):
        raise MagphaseHipError(
            "libmagphase_hip.so not found at %s -- build it with `python -m magphase_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().mpx_last_error()
        raise MagphaseHipError("%s failed (%d): %s" % (what, rc, msg.decode("utf-8", "replace") if msg else ""))
