"""Python host binding of libwce.so (the C ABI in include/wce.h).

Two layers, mirroring the C side:

* the reference's five entry points (main.c:4-8) with the same names and
  argument meaning -- one frame, host arrays, results written into H_EST --
  implemented by the compat shims in libwce.so (include/wce_compat.h);
* the batched engine: :class:`Context` (shared state on one device),
  :class:`DeviceArray` (HBM buffers), :meth:`Context.estimate` over B frames.

There is no CPU fallback: every compute call goes through the gfx950
kernels and raises :class:`WceError` if the library or the device is absent.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_double, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np

NSC = 53          # SAMPUTIL   (utils.h:13)
NBLK = 15         # OFDMBLK    (utils.h:15)
DC = 26           # main.c:74
PILOTS = (5, 19, 33, 47)   # utils.h:16-19

LT_LS = 1 << 0
PS_LINEAR = 1 << 1
PS_CUBIC = 1 << 2
PS_SINC = 1 << 3
PS_MMSE = 1 << 4
EQUALIZE = 1 << 5
LS_ALL = 0xF
ALL = 0x3F
OUT_LS_F32 = 1         # wce_outputs.flags: LS family + eq stored as complex float
FRAME_COV = 1 << 6   # WCE_MMSE_FRAME_COV: PS_MMSE covariance from each frame's own preamble
# the estimators, by result name and mask bit, in the order of wce_outputs' pointers
_ESTIMATORS = (("lt_ls", LT_LS), ("ps_linear", PS_LINEAR), ("ps_cubic", PS_CUBIC), ("ps_sinc", PS_SINC),
               ("ps_mmse", PS_MMSE))

MMSE_REF = 0
MMSE_TEXTBOOK = 1
MMSE_COV = 2       # TEXTBOOK with a caller-supplied channel covariance Rhh
FFT_SIZE = 64            # front end: 64-point DFT per OFDM block (WiFi_RX.m:10)
SAMPLES_PER_BLOCK = 80   # 64 + 16-sample cyclic prefix (WiFi_RX.m:12)
STF_LEN = 160            # short training field: ten periods of 16 samples (wce_short_field)
SEM_C = 0          # main.c semantics
SEM_MATLAB = 1     # WiFi_channel_estimation_*.m semantics
MOD_BPSK, MOD_QPSK, MOD_QAM16, MOD_QAM64 = 1, 2, 4, 6   # wce_demod.modulation: bits per data symbol
COMBINE_MAX_BRANCHES = 8   # WCE_COMBINE_MAX_BRANCHES: antennas wce_combine and wce_sync_share take
DEMOD_TRACK = 1 << 0     # remove each block's common pilot phase
DEMOD_REF_TX = 1 << 1    # EVM against tx instead of the decided point
TRACK_PHASE = 1 << 0     # WCE_TRACK_PHASE: per-block common pilot phase, as DEMOD_TRACK
TRACK_REF_TX = 1 << 1    # WCE_TRACK_REF_TX: EVM against tx, as DEMOD_REF_TX
TRACK_KNOWN_TX = 1 << 2  # WCE_TRACK_KNOWN_TX: the data-aided bound, nothing decided is fed back
RATE_1_2, RATE_2_3, RATE_3_4 = 0, 1, 2   # WCE_RATE_*: code rate of wce_viterbi_decode
DEC_TERMINATED = 1 << 0  # WCE_DEC_TERMINATED: trace back from state 0

STATUS = {0: "ok", -1: "invalid argument", -2: "HIP error", -3: "out of memory",
          -4: "context state not ready", -5: "no gfx950 device"}

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwce.so")


class WceError(RuntimeError):
    def __init__(self, code, where=""):
        msg = STATUS.get(code, f"error {code}")
        detail = ""
        if _lib is not None:
            try:
                detail = _lib.wce_last_error().decode()
            except Exception:  # pragma: no cover
                detail = ""
        super().__init__(f"{where}: {msg}" + (f" ({detail})" if detail else ""))
        self.code = code


class Complex(ctypes.Structure):
    _fields_ = [("re", c_double), ("im", c_double)]


class Frames(ctypes.Structure):
    """struct wce_frames (include/wce.h)."""
    _fields_ = [("tx", c_void_p), ("rx", c_void_p), ("rx_pre", c_void_p), ("tx_pre", c_void_p),
                ("frame_stride", c_int64), ("block_stride", c_int64), ("pre_stride", c_int64),
                ("n_frames", c_int64), ("block", c_int32), ("semantics", c_int32)]


class Outputs(ctypes.Structure):
    """struct wce_outputs (include/wce.h)."""
    _fields_ = [("lt_ls", c_void_p), ("ps_linear", c_void_p), ("ps_cubic", c_void_p), ("ps_sinc", c_void_p),
                ("ps_mmse", c_void_p), ("eq", c_void_p), ("out_stride", c_int64),
                ("eq_frame_stride", c_int64), ("eq_block_stride", c_int64), ("eq_source", c_uint32),
                ("flags", c_uint32)]


class Demod(ctypes.Structure):
    """struct wce_demod (include/wce.h)."""
    _fields_ = [("h", c_void_p), ("h_lt", c_void_p), ("h_stride", c_int64), ("modulation", c_int32),
                ("flags", c_uint32), ("scale", c_double)]


class DemodOut(ctypes.Structure):
    """struct wce_demod_out (include/wce.h)."""
    _fields_ = [("eq", c_void_p), ("sym", c_void_p), ("theta", c_void_p), ("evm", c_void_p), ("nerr", c_void_p),
                ("eq_frame_stride", c_int64), ("eq_block_stride", c_int64), ("sym_frame_stride", c_int64),
                ("sym_block_stride", c_int64)]


class Track(ctypes.Structure):
    """struct wce_track (include/wce.h)."""
    _fields_ = [("h", c_void_p), ("h_stride", c_int64), ("modulation", c_int32), ("flags", c_uint32),
                ("scale", c_double), ("mu", c_double), ("beta", c_int32)]


class TrackOut(ctypes.Structure):
    """struct wce_track_out (include/wce.h)."""
    _fields_ = [("eq", c_void_p), ("sym", c_void_p), ("theta", c_void_p), ("evm", c_void_p), ("nerr", c_void_p),
                ("eq_frame_stride", c_int64), ("eq_block_stride", c_int64), ("sym_frame_stride", c_int64),
                ("sym_block_stride", c_int64), ("h_blocks", c_void_p), ("hb_frame_stride", c_int64),
                ("hb_block_stride", c_int64), ("h_last", c_void_p), ("h_last_stride", c_int64)]


class CombinePar(ctypes.Structure):
    """struct wce_combine_par (include/wce.h)."""
    _fields_ = [("rx", c_void_p), ("rx_branch_stride", c_int64), ("rx_frame_stride", c_int64),
                ("rx_block_stride", c_int64), ("h", c_void_p), ("h_branch_stride", c_int64), ("h_stride", c_int64),
                ("ow2", c_void_p), ("ow2_branch_stride", c_int64), ("n_branches", c_int32)]


class CombineOut(ctypes.Structure):
    """struct wce_combine_out (include/wce.h)."""
    _fields_ = [("rx", c_void_p), ("rx_frame_stride", c_int64), ("rx_block_stride", c_int64), ("h", c_void_p),
                ("h_stride", c_int64)]


class ReencodePar(ctypes.Structure):
    """struct wce_reencode_par (include/wce.h)."""
    _fields_ = [("bits", c_void_p), ("bits_stride", c_int64), ("modulation", c_int32), ("rate", c_int32),
                ("scale", c_double), ("theta", c_void_p)]


class ReencodeOut(ctypes.Structure):
    """struct wce_reencode_out (include/wce.h)."""
    _fields_ = [("tx", c_void_p), ("tx_frame_stride", c_int64), ("tx_block_stride", c_int64), ("h", c_void_p),
                ("h_stride", c_int64)]


class PsduPar(ctypes.Structure):
    """struct wce_psdu_par (include/wce.h)."""
    _fields_ = [("modulation", c_int32), ("rate", c_int32), ("length", c_int32), ("seed", c_int32),
                ("lengths", c_void_p), ("seeds", c_void_p)]


class PsduOut(ctypes.Structure):
    """struct wce_psdu_out (include/wce.h)."""
    _fields_ = [("psdu", c_void_p), ("psdu_stride", c_int64), ("seed", c_void_p), ("fcs_ok", c_void_p),
                ("n_good", c_void_p)]


class ChannelPar(ctypes.Structure):
    """struct wce_channel_par (include/wce.h)."""
    _fields_ = [("taps", c_void_p), ("taps_stride", c_int64), ("n_taps", c_int32), ("field", c_int32),
                ("cfo", c_void_p), ("ow2", c_void_p), ("delay", c_void_p), ("seed", c_uint64),
                ("first_frame", c_int64)]


class FadingPar(ctypes.Structure):
    """struct wce_fading_par (include/wce.h)."""
    _fields_ = [("knots", c_void_p), ("frame_stride", c_int64), ("knot_stride", c_int64), ("n_knots", c_int32),
                ("knot_period", c_int32), ("n_taps", c_int32), ("field", c_int32), ("cfo", c_void_p),
                ("ow2", c_void_p), ("delay", c_void_p), ("seed", c_uint64), ("first_frame", c_int64)]


_lib = None

# (name, argtypes) for every symbol include/wce.h and include/wce_compat.h declare
ABI = {
    "wce_ctx_create": [POINTER(c_void_p), c_int, c_void_p, c_void_p, c_double, c_int],
    "wce_ctx_create_empty": [POINTER(c_void_p), c_int],
    "wce_ctx_destroy": [c_void_p],
    "wce_ctx_reserve": [c_void_p, c_int64],
    "wce_ctx_reserve_stream": [c_void_p, c_int64, c_void_p],
    "wce_plan_create": [POINTER(c_void_p), c_void_p, c_void_p, c_void_p, c_uint32],
    "wce_plan_launch": [c_void_p, c_void_p],
    "wce_plan_destroy": [c_void_p],
    "wce_ctx_create_cov": [POINTER(c_void_p), c_int, c_void_p, c_void_p, c_void_p, c_double],
    "wce_state_build_cov": [c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_double],
    "wce_debug_set_fusion": [c_void_p, c_int],
    "wce_debug_set_border_dot": [c_void_p, c_int],
    "wce_debug_set_flat_chunk": [ctypes.c_int64],
    "wce_debug_set_variant": [c_int, c_int],
    "wce_debug_chain_grid": [c_int64, c_int64],
    "wce_debug_rank1_rows_per_sweep": [c_void_p],
    "wce_debug_rank1_head": [c_int] * 7 + [c_int64] * 3 + [c_int, POINTER(c_int)],
    "wce_debug_rank1_head_groups": [c_uint32, c_uint32, POINTER(c_uint32), c_uint32],
    "wce_debug_set_cov_path": [c_void_p, c_int],
    "wce_debug_lr_kernel": [c_void_p, c_int64],
    "wce_debug_route": [c_int] * 7 + [c_uint32] + [c_int] * 4 + [ctypes.c_char_p, c_size_t],
    "wce_debug_route_noise": [c_int] * 7 + [c_uint32] + [c_int] * 5 + [ctypes.c_char_p, c_size_t],
    "wce_debug_cov_factor": [c_void_p, c_size_t, c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_double),
                             POINTER(c_double)],
    "wce_ctx_cov_info": [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_double), POINTER(c_double)],
    "wce_ctx_set_modulus": [c_void_p, c_void_p],
    "wce_state_set_modulus": [c_void_p, c_size_t, c_void_p, c_void_p],
    "wce_debug_set_cm": [c_void_p, c_int],
    "wce_debug_compat_state_builds": [],
    "wce_ctx_state": [c_void_p, POINTER(c_void_p), POINTER(c_size_t)],
    "wce_ctx_mark_ready": [c_void_p],
    "wce_state_size": [],
    "wce_state_build": [c_void_p, c_size_t, c_void_p, c_void_p, c_double, c_int],
    "wce_ctx_load_state": [c_void_p, c_void_p, c_size_t],
    "wce_state_validate": [c_void_p, c_size_t, POINTER(c_int)],
    "wce_ctx_get_shared": [c_void_p, c_void_p, c_void_p, POINTER(c_double), POINTER(c_double)],
    "wce_estimate": [c_void_p, POINTER(Frames), POINTER(Outputs), c_uint32, c_void_p],
    "wce_estimate_noise": [c_void_p, POINTER(Frames), POINTER(Outputs), c_uint32, c_void_p, c_void_p],
    "wce_mmse_solve": [c_void_p, POINTER(Frames), c_void_p, c_int64, c_void_p],
    "wce_mmse_apply": [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p],
    "wce_synth_frames": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64,
                         c_uint64, c_void_p, c_double, c_double, c_void_p],
    "wce_front_end_blocks": [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int64, c_int64, c_void_p],
    "wce_front_end_preamble": [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                               c_void_p],
    "wce_front_end_blocks_cfo": [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_int64,
                                 c_int64, c_void_p],
    "wce_front_end_preamble_cfo": [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                   c_void_p, c_int, c_void_p],
    "wce_front_end_sync": [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_double, c_int32, c_void_p,
                           c_void_p, c_void_p],
    "wce_front_end_sync_stf": [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_double, c_double, c_int32,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "wce_short_field": [c_void_p, c_double, c_void_p, c_int64, c_int64, c_void_p],
    "wce_debug_short_field_period": [c_void_p],
    "wce_debug_sync_stf_tiles": [POINTER(c_int), POINTER(c_int)],
    "wce_front_end_preamble_at": [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                  c_void_p, c_void_p, c_int, c_void_p],
    "wce_front_end_blocks_at": [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_int64,
                                c_void_p, c_int64, c_int64, c_void_p],
    "wce_demodulate": [c_void_p, POINTER(Frames), POINTER(Demod), POINTER(DemodOut), c_void_p],
    "wce_track_demodulate": [c_void_p, POINTER(Frames), POINTER(Track), POINTER(TrackOut), c_void_p],
    "wce_combine": [c_void_p, POINTER(CombinePar), c_int64, POINTER(CombineOut), c_void_p],
    "wce_sync_share": [c_void_p, c_int32, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p],
    "wce_soft_demap_blocks": [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int32, c_double,
                              c_int64, c_void_p, c_int64, c_int64, c_void_p],
    "wce_soft_demap": [c_void_p, c_void_p, c_int64, c_int64, POINTER(Demod), c_int64, c_void_p, c_int64, c_int64,
                       c_void_p],
    "wce_viterbi_decode": [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_uint32, c_int64, c_void_p,
                           c_int64, c_void_p, c_int64, c_void_p, c_void_p],
    "wce_decode_info_bits": [c_int32, c_int32],
    "wce_reencode": [c_void_p, POINTER(ReencodePar), POINTER(Frames), c_int64, POINTER(ReencodeOut), c_void_p],
    "wce_psdu_max_len": [c_int32, c_int32],
    "wce_psdu_frame": [c_void_p, POINTER(PsduPar), c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p],
    "wce_psdu_deframe": [c_void_p, POINTER(PsduPar), c_void_p, c_int64, c_int64, POINTER(PsduOut), c_void_p],
    "wce_modulate": [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int64, c_void_p, c_int64,
                     c_void_p],
    "wce_channel": [c_void_p, c_void_p, c_int64, c_int64, c_int64, POINTER(ChannelPar), c_void_p, c_int64, c_int64,
                    c_void_p],
    "wce_transmit": [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int64, POINTER(ChannelPar),
                     c_void_p, c_int64, c_int64, c_void_p],
    "wce_channel_tv": [c_void_p, c_void_p, c_int64, c_int64, c_int64, POINTER(FadingPar), c_void_p, c_int64, c_int64,
                       c_void_p],
    "wce_transmit_tv": [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int64,
                        POINTER(FadingPar), c_void_p, c_int64, c_int64, c_void_p],
    "wce_nonfinite_scan": [c_void_p, c_void_p, ctypes.c_int64, ctypes.c_int64, c_uint32, c_void_p, c_void_p,
                           c_void_p],
    "wce_comm_unique_id": [c_void_p],
    "wce_comm_init_rank": [POINTER(c_void_p), c_void_p, c_int, c_int, c_int],
    "wce_comm_init_all": [POINTER(c_void_p), c_int, POINTER(c_int)],
    "wce_comm_destroy": [c_void_p],
    "wce_comm_info": [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int)],
    "wce_ctx_broadcast_state": [c_void_p, c_void_p, c_int, c_void_p],
    "wce_ctx_broadcast_state_all": [POINTER(c_void_p), POINTER(c_void_p), c_int, c_int, POINTER(c_void_p)],
    "wce_comm_max_f64": [c_void_p, POINTER(c_double), c_void_p],
    "wce_comm_max_f64_all": [POINTER(c_void_p), c_int, POINTER(c_double), POINTER(c_void_p)],
    "wce_shard": [ctypes.c_int64, c_int, c_int, POINTER(ctypes.c_int64), POINTER(ctypes.c_int64)],
    "wce_device_count": [POINTER(c_int)],
    "wce_set_device": [c_int],
    "wce_malloc": [POINTER(c_void_p), c_size_t],
    "wce_free": [c_void_p],
    "wce_memcpy_htod": [c_void_p, c_void_p, c_size_t],
    "wce_memcpy_dtoh": [c_void_p, c_void_p, c_size_t],
    "wce_memcpy_dtod": [c_void_p, c_void_p, c_size_t, c_void_p],
    "wce_ldc_to_complex": [c_void_p, c_void_p, ctypes.c_int64, c_void_p],
    "wce_complex_to_ldc": [c_void_p, c_void_p, ctypes.c_int64, c_void_p],
    "wce_memset": [c_void_p, c_int, c_size_t],
    "wce_host_alloc": [POINTER(c_void_p), c_size_t],
    "wce_host_free": [c_void_p],
    "wce_memcpy_htod_async": [c_void_p, c_void_p, c_size_t, c_void_p],
    "wce_memcpy_dtoh_async": [c_void_p, c_void_p, c_size_t, c_void_p],
    "wce_stream_create": [POINTER(c_void_p)],
    "wce_stream_destroy": [c_void_p],
    "wce_stream_synchronize": [c_void_p],
    "wce_event_create": [POINTER(c_void_p)],
    "wce_event_destroy": [c_void_p],
    "wce_event_record": [c_void_p, c_void_p],
    "wce_event_query": [c_void_p],
    "wce_event_elapsed_ms": [POINTER(ctypes.c_float), c_void_p, c_void_p],
    "wce_last_error": [],
    "wce_version": [],
    "wce_compat_last_status": [],
    "WiFi_channel_estimation_LT_LS": [c_void_p, c_void_p, c_void_p],
    "WiFi_channel_estimation_PS_Linear": [c_void_p, c_void_p, c_void_p],
    "WiFi_channel_estimation_PS_Cubic": [c_void_p, c_void_p, c_void_p],
    "WiFi_channel_estimation_PS_Sinc": [c_void_p, c_void_p, c_void_p],
    "WiFi_channel_estimation_PS_MMSE": [c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p],
}
_VOID = {"WiFi_channel_estimation_LT_LS", "WiFi_channel_estimation_PS_Linear", "WiFi_channel_estimation_PS_Cubic",
         "WiFi_channel_estimation_PS_Sinc", "WiFi_channel_estimation_PS_MMSE"}
_STR = {"wce_last_error", "wce_version", "wce_debug_lr_kernel"}


def load(path: str = LIB_PATH):
    """Load libwce.so (in-tree build).  Raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise WceError(-5, f"libwce.so not built at {path}; run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    for name, args in ABI.items():
        if name.startswith("wce_debug_") and not hasattr(lib, name):
            continue   # debug hooks are optional (older builds in A/B harnesses)
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = None if name in _VOID else (ctypes.c_char_p if name in _STR else c_int)
    lib.wce_state_size.restype = c_size_t
    if hasattr(lib, "wce_debug_compat_state_builds"):
        lib.wce_debug_compat_state_builds.restype = ctypes.c_ulonglong
    if hasattr(lib, "wce_debug_chain_grid"):
        lib.wce_debug_chain_grid.restype = c_int64
    _lib = lib
    return lib


def _check(rc, where):
    if rc != 0:
        raise WceError(rc, where)


def info_bits(modulation, rate) -> int:
    """wce_decode_info_bits: information bits (trellis steps) per frame of 15 blocks, 48 data subcarriers each."""
    T = load().wce_decode_info_bits(int(modulation), int(rate))
    if T < 0:
        raise WceError(T, "wce_decode_info_bits")
    return T


def psdu_max_len(modulation, rate) -> int:
    """wce_psdu_max_len: the longest PSDU, FCS included, a frame of `modulation` at `rate` carries:
    (info_bits - 22) // 8 octets."""
    n = load().wce_psdu_max_len(int(modulation), int(rate))
    if n < 0:
        raise WceError(n, "wce_psdu_max_len")
    return n


def device_count() -> int:
    n = c_int(0)
    _check(load().wce_device_count(byref(n)), "wce_device_count")
    return n.value


def _as_c128(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.complex128))


class PinnedArray:
    """Page-locked host memory (wce_host_alloc) with a numpy view, for
    stream-ordered copies that overlap estimation."""

    def __init__(self, shape, dtype=np.complex128):
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = c_void_p()
        _check(load().wce_host_alloc(byref(self.ptr), max(self.nbytes, 16)), "wce_host_alloc")
        buf = (ctypes.c_char * max(self.nbytes, 16)).from_address(self.ptr.value)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(np.prod(self.shape))).reshape(self.shape)

    @property
    def addr(self) -> int:
        return self.ptr.value

    def free(self):
        if self.ptr is not None and self.ptr.value:
            self.array = None
            _lib.wce_host_free(self.ptr)
            self.ptr = c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:  # pragma: no cover
            pass


class DeviceArray:
    """A complex128 buffer in HBM (owned)."""

    def __init__(self, shape, dtype=np.complex128, zero=False):
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = c_void_p()
        _check(load().wce_malloc(byref(self.ptr), max(self.nbytes, 16)), "wce_malloc")
        if zero:
            _check(_lib.wce_memset(self.ptr, 0, max(self.nbytes, 16)), "wce_memset")

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        d = cls(a.shape, a.dtype)
        if d.nbytes:
            _check(_lib.wce_memcpy_htod(d.ptr, a.ctypes.data_as(c_void_p), d.nbytes), "wce_memcpy_htod")
        return d

    def numpy(self) -> np.ndarray:
        out = np.empty(self.shape, self.dtype)
        if self.nbytes:
            _check(_lib.wce_memcpy_dtoh(out.ctypes.data_as(c_void_p), self.ptr, self.nbytes), "wce_memcpy_dtoh")
        return out

    def rows(self, first, count=1) -> np.ndarray:
        """rows [first, first + count) of the leading axis, without copying the rest"""
        first, count = int(first), int(count)
        if first < 0 or count < 0 or first + count > self.shape[0]:
            raise IndexError("rows out of range")
        out = np.empty((count,) + self.shape[1:], self.dtype)
        row = out.nbytes // max(count, 1)
        if out.nbytes:
            _check(_lib.wce_memcpy_dtoh(out.ctypes.data_as(c_void_p), c_void_p(self.addr + first * row), out.nbytes),
                   "wce_memcpy_dtoh")
        return out

    def free(self):
        if self.ptr is not None and self.ptr.value:
            _lib.wce_free(self.ptr)
            self.ptr = c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:  # pragma: no cover
            pass

    @property
    def addr(self) -> int:
        return self.ptr.value or 0


def _addr(x):
    if x is None:
        return None
    if isinstance(x, DeviceArray):
        return x.addr
    return int(x)


class Context:
    """wce_ctx: shared (frame-independent) state resident on one device."""

    def __init__(self, tx_pre=None, rx_pre=None, ow2=None, mode=MMSE_REF, device=0, empty=False, Rhh=None):
        lib = load()
        self.handle = c_void_p()
        self.device = device
        self.mode = MMSE_COV if Rhh is not None else mode
        self.tx_pre = None
        if empty:
            _check(lib.wce_ctx_create_empty(byref(self.handle), device), "wce_ctx_create_empty")
            return
        tp, rp = _as_c128(tx_pre), _as_c128(rx_pre)
        if tp.shape != (NSC,) or rp.shape != (NSC,):
            raise ValueError("tx_pre / rx_pre must hold 53 subcarriers")
        self.tx_pre = tp.copy()   # link_host transmits it
        if Rhh is not None:   # WCE_MMSE_COV: model channel covariance (53 x 53, time domain)
            R = _as_c128(Rhh)
            if R.shape != (NSC, NSC):
                raise ValueError("Rhh must be 53 x 53")
            _check(lib.wce_ctx_create_cov(byref(self.handle), device, tp.ctypes.data_as(c_void_p),
                                          rp.ctypes.data_as(c_void_p), R.ctypes.data_as(c_void_p), float(ow2)),
                   "wce_ctx_create_cov")
            return
        _check(lib.wce_ctx_create(byref(self.handle), device, tp.ctypes.data_as(c_void_p),
                                  rp.ctypes.data_as(c_void_p), float(ow2), mode), "wce_ctx_create")

    def set_fusion(self, on: bool):
        """A/B switch: LS family + equalization fused into the MMSE solve (default on)."""
        _check(_lib.wce_debug_set_fusion(self.handle, int(bool(on))), "wce_debug_set_fusion")

    def plan(self, frames: "Frames", outputs: "Outputs", mask: int) -> "Plan":
        """Capture one estimate call into a HIP graph (wce_plan_create)."""
        return Plan(self, frames, outputs, mask)

    def cov_info(self):
        """WCE_MMSE_COV: (rank r, low-rank path taken, lambda_max, lambda_min of the kept spectrum of C)."""
        r, lr = c_int(), c_int()
        lmax, lmin = c_double(), c_double()
        _check(load().wce_ctx_cov_info(self.handle, ctypes.byref(r), ctypes.byref(lr), ctypes.byref(lmax),
                                       ctypes.byref(lmin)), "cov_info")
        return r.value, bool(lr.value), lmax.value, lmin.value

    def set_modulus(self, x_ref):
        """WCE_MMSE_COV: the constant-modulus operator for frames with |x|^2 = |x_ref|^2 (None: off)."""
        if x_ref is None:
            _check(load().wce_ctx_set_modulus(self.handle, None), "wce_ctx_set_modulus")
            return
        x = _as_c128(x_ref)
        if x.shape != (NSC,):
            raise ValueError("x_ref must hold 53 subcarriers")
        _check(load().wce_ctx_set_modulus(self.handle, x.ctypes.data_as(c_void_p)), "wce_ctx_set_modulus")

    def set_cm(self, on: bool):
        """A/B switch of the constant-modulus path (default on once a pattern is set)."""
        _check(load().wce_debug_set_cm(self.handle, int(bool(on))), "wce_debug_set_cm")

    def set_cov_path(self, path: int):
        """A/B: 0 = the state's choice, 1 = dense Ryy solve, 2 = low-rank Gram path."""
        _check(load().wce_debug_set_cov_path(self.handle, path), "set_cov_path")

    def lr_kernel(self, units: int) -> str:
        """The low-rank kernel an estimate over `units` (frame, block) units runs ("" on the dense path)."""
        return load().wce_debug_lr_kernel(self.handle, int(units)).decode()

    def set_border_dot(self, on: bool):
        """A/B switch: rank-1 covariance via a second bordered row (default on)."""
        _check(_lib.wce_debug_set_border_dot(self.handle, int(bool(on))), "wce_debug_set_border_dot")

    def reserve(self, n_frames):
        """Pre-size the WCE_MMSE_FRAME_COV workspace (no allocation inside estimate)."""
        _check(_lib.wce_ctx_reserve(self.handle, n_frames), "wce_ctx_reserve")

    def close(self):
        if self.handle is not None and self.handle.value:
            _lib.wce_ctx_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass

    def state(self):
        ptr, nb = c_void_p(), c_size_t()
        _check(_lib.wce_ctx_state(self.handle, byref(ptr), byref(nb)), "wce_ctx_state")
        return ptr.value, nb.value

    def load_state(self, blob: np.ndarray):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        _check(_lib.wce_ctx_load_state(self.handle, blob.ctypes.data_as(c_void_p), blob.nbytes),
               "wce_ctx_load_state")

    def mark_ready(self):
        _check(_lib.wce_ctx_mark_ready(self.handle), "wce_ctx_mark_ready")

    def shared(self):
        h = np.zeros(NSC, np.complex128)
        C = np.zeros((NSC, NSC), np.complex128)
        a, b = c_double(), c_double()
        _check(_lib.wce_ctx_get_shared(self.handle, h.ctypes.data_as(c_void_p), C.ctypes.data_as(c_void_p),
                                       byref(a), byref(b)), "wce_ctx_get_shared")
        return h, C, a.value, b.value

    # ---------------------------------------------------------------- batched
    @staticmethod
    def frames(tx, rx, n_frames, frame_stride=NBLK * NSC, block_stride=NSC, rx_pre=None, pre_stride=NSC,
               tx_pre=None, block=0, semantics=SEM_C) -> Frames:
        return Frames(_addr(tx), _addr(rx), _addr(rx_pre), _addr(tx_pre), frame_stride, block_stride, pre_stride,
                      n_frames, block, semantics)

    def nonfinite_scan(self, H, n_frames, stride=NSC, f32=False, bitmap=None, n_bad=None, stream=None):
        """wce_nonfinite_scan on a device output array.  With bitmap/n_bad
        None, allocates them, waits, and returns (bitmap as numpy uint32,
        number of non-finite frames); otherwise enqueues into the given
        device buffers and returns None."""
        own = bitmap is None
        if own:
            bitmap = DeviceArray(((n_frames + 31) // 32,), dtype=np.uint32)
            n_bad = DeviceArray((1,), dtype=np.uint64)
        _check(_lib.wce_nonfinite_scan(self.handle, _addr(H), stride, n_frames, OUT_LS_F32 if f32 else 0, _addr(bitmap),
                                       _addr(n_bad), stream), "wce_nonfinite_scan")
        if not own:
            return None
        if stream is not None:
            _check(_lib.wce_stream_synchronize(stream), "wce_stream_synchronize")
        return bitmap.numpy(), int(n_bad.numpy()[0])

    def estimate(self, frames: Frames, outputs: Outputs, mask: int, stream=None, ow2=None):
        """wce_estimate; ow2 (a device array of n_frames doubles, e.g. front_end_preamble's): wce_estimate_noise,
        each frame's PS_MMSE with its own noise variance (TEXTBOOK contexts)."""
        if ow2 is None:
            _check(_lib.wce_estimate(self.handle, byref(frames), byref(outputs), mask, stream), "wce_estimate")
            return
        _check(_lib.wce_estimate_noise(self.handle, byref(frames), byref(outputs), mask, _addr(ow2), stream),
               "wce_estimate_noise")

    def demodulate(self, frames: Frames, h, h_lt=None, h_stride=NSC, modulation=MOD_BPSK, scale=8.8753, track=True,
                   ref_tx=True, eq=None, sym=None, theta=None, evm=None, nerr=None, stream=None,
                   eq_frame_stride=None, eq_block_stride=NSC, sym_frame_stride=None, sym_block_stride=NSC):
        """wce_demodulate on device arrays: equalize `frames` with the estimate h [n][h_stride] (blended with
        h_lt over the blocks, if given), remove each block's common pilot phase (track), slice to `modulation`
        and score.  Outputs, each optional: eq complex [n][15][53], sym uint8 [n][15][53] (Gray labels, 0xFF
        where the symbol is not finite), theta float64 [n][15], evm float64 [n] (against tx with ref_tx, else
        against the decided points), nerr uint32 [n].  Frame strides default to 15 block strides."""
        p = Demod(_addr(h), _addr(h_lt), h_stride, modulation,
                  (DEMOD_TRACK if track else 0) | (DEMOD_REF_TX if ref_tx else 0), scale)
        o = DemodOut(_addr(eq), _addr(sym), _addr(theta), _addr(evm), _addr(nerr),
                     eq_frame_stride if eq_frame_stride is not None else NBLK * eq_block_stride, eq_block_stride,
                     sym_frame_stride if sym_frame_stride is not None else NBLK * sym_block_stride, sym_block_stride)
        _check(_lib.wce_demodulate(self.handle, byref(frames), byref(p), byref(o), stream), "wce_demodulate")

    def _demod_device(self, fr, B, dh, dhlt, modulation, scale, track, ref_tx):
        """queue demodulate with every output; -> name -> DeviceArray (read them after a synchronize)"""
        d = {"eq": DeviceArray((B, NBLK, NSC), zero=True), "sym": DeviceArray((B, NBLK, NSC), np.uint8, zero=True),
             "theta": DeviceArray((B, NBLK), np.float64, zero=True), "evm": DeviceArray((B,), np.float64, zero=True),
             "nerr": DeviceArray((B,), np.uint32, zero=True)}
        self.demodulate(fr, dh, dhlt, NSC, modulation, scale, track, ref_tx, **d)
        return d

    def demodulate_host(self, tx, rx, h, h_lt=None, modulation=MOD_BPSK, scale=8.8753, track=True, ref_tx=True):
        """Convenience: host frames [B][15][53] and estimates h (and h_lt) [B][53] -> dict of host arrays
        eq, sym, theta, evm, nerr."""
        tx, rx, h = _as_c128(tx), _as_c128(rx), _as_c128(h)
        B = tx.shape[0]
        if tx.shape != (B, NBLK, NSC) or rx.shape != tx.shape:
            raise ValueError("tx/rx must be [B][15][53] complex")
        if h.shape != (B, NSC) or (h_lt is not None and np.shape(h_lt) != (B, NSC)):
            raise ValueError("h / h_lt must be [B][53] complex")
        dtx, drx, dh = DeviceArray.from_numpy(tx), DeviceArray.from_numpy(rx), DeviceArray.from_numpy(h)
        dhlt = DeviceArray.from_numpy(_as_c128(h_lt)) if h_lt is not None else None
        d = self._demod_device(self.frames(dtx, drx, B), B, dh, dhlt, modulation, scale, track, ref_tx)
        synchronize()
        return {n: a.numpy() for n, a in d.items()}

    def track_demodulate(self, frames: Frames, h, mu, beta, h_stride=NSC, modulation=MOD_BPSK, scale=8.8753,
                         phase=True, ref_tx=True, known_tx=False, eq=None, sym=None, theta=None, evm=None, nerr=None,
                         h_blocks=None, h_last=None, stream=None, eq_frame_stride=None, eq_block_stride=NSC,
                         sym_frame_stride=None, sym_block_stride=NSC, hb_frame_stride=None, hb_block_stride=NSC,
                         h_last_stride=NSC):
        """wce_track_demodulate on device arrays: demodulate `frames` block by block, starting each frame from the
        estimate h [n][h_stride] and re-estimating the channel after every block from the decided symbols (the
        tx symbols with known_tx: the data-aided bound), averaged over the 2 beta + 1 neighbouring subcarriers
        (beta 0..4) and moved towards that by the time weight mu (0..1; 0: h throughout).  phase, ref_tx: as
        demodulate's track and ref_tx.  Outputs, each optional: demodulate's eq, sym, theta, evm and nerr; h_blocks
        complex [n][15][hb_block_stride], the estimate each block was equalized with (soft_demap_blocks reads
        it); h_last complex [n][h_last_stride], the estimate after the last block.  Frame strides default to 15
        block strides."""
        p = Track(_addr(h), h_stride, modulation, (TRACK_PHASE if phase else 0) | (TRACK_REF_TX if ref_tx else 0) |
                  (TRACK_KNOWN_TX if known_tx else 0), scale, mu, beta)
        o = TrackOut(_addr(eq), _addr(sym), _addr(theta), _addr(evm), _addr(nerr),
                     eq_frame_stride if eq_frame_stride is not None else NBLK * eq_block_stride, eq_block_stride,
                     sym_frame_stride if sym_frame_stride is not None else NBLK * sym_block_stride, sym_block_stride,
                     _addr(h_blocks), hb_frame_stride if hb_frame_stride is not None else NBLK * hb_block_stride,
                     hb_block_stride, _addr(h_last), h_last_stride)
        _check(_lib.wce_track_demodulate(self.handle, byref(frames), byref(p), byref(o), stream),
               "wce_track_demodulate")

    def _track_device(self, fr, B, dh, mu, beta, modulation, scale, phase, ref_tx, known_tx=False):
        """queue track_demodulate with every output; -> name -> DeviceArray (read them after a synchronize)"""
        d = {"eq": DeviceArray((B, NBLK, NSC), zero=True), "sym": DeviceArray((B, NBLK, NSC), np.uint8, zero=True),
             "theta": DeviceArray((B, NBLK), np.float64, zero=True), "evm": DeviceArray((B,), np.float64, zero=True),
             "nerr": DeviceArray((B,), np.uint32, zero=True), "h_blocks": DeviceArray((B, NBLK, NSC), zero=True),
             "h_last": DeviceArray((B, NSC), zero=True)}
        self.track_demodulate(fr, dh, mu, beta, NSC, modulation, scale, phase, ref_tx, known_tx, **d)
        return d

    def _track_inputs(self, tx, rx, h):
        """host frames [B][15][53] and estimates [B][53], checked, on the device -> (B, frames, keep)"""
        tx, rx, h = _as_c128(tx), _as_c128(rx), _as_c128(h)
        B = tx.shape[0]
        if tx.shape != (B, NBLK, NSC) or rx.shape != tx.shape:
            raise ValueError("tx/rx must be [B][15][53] complex")
        if h.shape != (B, NSC):
            raise ValueError("h must be [B][53] complex")
        keep = [DeviceArray.from_numpy(tx), DeviceArray.from_numpy(rx), DeviceArray.from_numpy(h)]
        return B, self.frames(keep[0], keep[1], B), keep

    def track_demodulate_host(self, tx, rx, h, mu=0.5, beta=2, modulation=MOD_BPSK, scale=8.8753, phase=True,
                              ref_tx=True, known_tx=False):
        """Convenience: host frames [B][15][53] and starting estimates h [B][53] -> dict of host arrays eq, sym,
        theta, evm, nerr (as demodulate_host), h_blocks [B][15][53] and h_last [B][53]."""
        B, fr, keep = self._track_inputs(tx, rx, h)
        d = self._track_device(fr, B, keep[2], mu, beta, modulation, scale, phase, ref_tx, known_tx)
        synchronize()
        return {n: a.numpy() for n, a in d.items()}

    def track_decode_host(self, tx, rx, h, modulation=MOD_BPSK, rate=RATE_1_2, mu=0.5, beta=2, scale=8.8753,
                          phase=True, terminated=True, ref_bits=None):
        """Convenience: the tracked receive chain on host frames [B][15][53] and starting estimates h [B][53]:
        track_demodulate, soft_demap_blocks on its eq and h_blocks, viterbi_decode at `rate`, queued on one stream
        with no host hop between them -> dict of host arrays: "demod" (the dict of track_demodulate_host), llr
        float32 [B][15][48 * modulation], bits uint8 [B][T] and, with ref_bits [B][T], nbiterr uint32 [B]."""
        B, fr, keep = self._track_inputs(tx, rx, h)
        trk = self._track_device(fr, B, keep[2], mu, beta, modulation, scale, phase, True)
        d = self._decode_device(trk["eq"], None, None, B, modulation, rate, scale, terminated, ref_bits,
                                h_blocks=trk["h_blocks"])
        synchronize()
        res = self._decode_result(d, modulation, rate)
        res["demod"] = {n: a.numpy() for n, a in trk.items()}
        return res

    def soft_demap_blocks(self, eq, h_blocks, n_frames, modulation=MOD_BPSK, scale=8.8753, llr=None,
                          eq_frame_stride=None, eq_block_stride=NSC, hb_frame_stride=None, hb_block_stride=NSC,
                          llr_frame_stride=None, llr_block_stride=None, stream=None):
        """wce_soft_demap_blocks on device arrays: soft_demap with an estimate per block, h_blocks complex
        [n][15][hb_block_stride] (track_demodulate's): block b's soft bits are weighed by |h_blocks[b]|^2.  Where
        every block row of a frame is the same h the soft bits are soft_demap's with that h and no h_lt, bit for
        bit.  Strides as soft_demap."""
        lbs = llr_block_stride if llr_block_stride is not None else 48 * modulation
        _check(_lib.wce_soft_demap_blocks(self.handle, _addr(eq),
                                          eq_frame_stride if eq_frame_stride is not None else NBLK * eq_block_stride,
                                          eq_block_stride, _addr(h_blocks),
                                          hb_frame_stride if hb_frame_stride is not None else NBLK * hb_block_stride,
                                          hb_block_stride, modulation, scale, n_frames, _addr(llr),
                                          llr_frame_stride if llr_frame_stride is not None else NBLK * lbs, lbs,
                                          stream), "wce_soft_demap_blocks")

    def soft_demap(self, eq, h, n_frames, h_lt=None, h_stride=NSC, modulation=MOD_BPSK, scale=8.8753, llr=None,
                   eq_frame_stride=None, eq_block_stride=NSC, llr_frame_stride=None, llr_block_stride=None,
                   stream=None):
        """wce_soft_demap on device arrays: the equalized symbols eq complex [n][15][eq_block_stride] (e.g.
        demodulate's) and the estimate h [n][h_stride] (blended with h_lt over the blocks, if given, as
        demodulate blends) -> llr float32 [n][15][llr_block_stride]: per block the 48 * modulation max-log soft
        bits |Hu|^2 (D0 - D1) in deinterleaved coded order, > 0 for bit 1, 0 where eq or Hu is not finite.
        Block strides default to 53 and 48 * modulation, frame strides to 15 block strides."""
        lbs = llr_block_stride if llr_block_stride is not None else 48 * modulation
        p = Demod(_addr(h), _addr(h_lt), h_stride, modulation, 0, scale)
        _check(_lib.wce_soft_demap(self.handle, _addr(eq),
                                   eq_frame_stride if eq_frame_stride is not None else NBLK * eq_block_stride,
                                   eq_block_stride, byref(p), n_frames, _addr(llr),
                                   llr_frame_stride if llr_frame_stride is not None else NBLK * lbs, lbs, stream),
               "wce_soft_demap")

    def viterbi_decode(self, llr, n_frames, modulation, rate, terminated=True, bits=None, bits_stride=None,
                       ref_bits=None, ref_stride=None, nbiterr=None, llr_frame_stride=None, llr_block_stride=None,
                       stream=None):
        """wce_viterbi_decode on device arrays: llr float32 [n][15][llr_block_stride] (soft_demap's) of
        `modulation` at code rate `rate` (RATE_*) -> bits uint8 [n][bits_stride], the info_bits(modulation, rate)
        information bits packed LSB first, and/or nbiterr uint32 [n], the bits that differ from ref_bits (packed
        the same way, [n][ref_stride]).  terminated: the traceback starts from state 0.  The byte strides default
        to ceil(T / 8), the block stride to 48 * modulation, the frame stride to 15 block strides."""
        lbs = llr_block_stride if llr_block_stride is not None else 48 * modulation
        nbytes = (info_bits(modulation, rate) + 7) // 8
        _check(_lib.wce_viterbi_decode(self.handle, _addr(llr),
                                       llr_frame_stride if llr_frame_stride is not None else NBLK * lbs, lbs,
                                       modulation, rate, DEC_TERMINATED if terminated else 0, n_frames, _addr(bits),
                                       bits_stride if bits_stride is not None else nbytes, _addr(ref_bits),
                                       ref_stride if ref_stride is not None else nbytes, _addr(nbiterr), stream),
               "wce_viterbi_decode")

    def reencode(self, bits, n_frames, modulation, rate, scale=8.8753, bits_stride=None, theta=None, frames=None,
                 tx=None, tx_frame_stride=None, tx_block_stride=NSC, h=None, h_stride=NSC, stream=None):
        """wce_reencode on device arrays: bits uint8 [n][bits_stride] (viterbi_decode's packed information bits) of
        `modulation` at code rate `rate` -> tx complex [n][15][tx_block_stride], the symbols the transmitter sent
        for them (pilots copied from frames.tx where `frames` has one, else 802.11's; DC 0), and/or h complex
        [n][h_stride], the data-aided LS estimate sum_b conj(tx_b) rx_b r_b / sum_b |tx_b|^2 against frames.rx with
        the rotors r_b = exp(-i theta[n][b]) (theta float64 [n][15] as demodulate writes it; None: 1).  bits_stride
        defaults to ceil(T / 8), the tx frame stride to 15 block strides."""
        nbytes = (info_bits(modulation, rate) + 7) // 8
        p = ReencodePar(_addr(bits), bits_stride if bits_stride is not None else nbytes, modulation, rate, scale,
                        _addr(theta))
        o = ReencodeOut(_addr(tx), tx_frame_stride if tx_frame_stride is not None else NBLK * tx_block_stride,
                        tx_block_stride, _addr(h), h_stride)
        _check(_lib.wce_reencode(self.handle, byref(p), byref(frames) if frames is not None else None, n_frames,
                                 byref(o), stream), "wce_reencode")

    def psdu_frame(self, payload, n_frames, modulation, rate, length=None, lengths=None, seed=93, seeds=None,
                   bits=None, payload_stride=None, bits_stride=None, stream=None):
        """wce_psdu_frame on device arrays: payload uint8 [n][payload_stride], the PSDU octets in front of the FCS
        (length - 4 of them; None where every frame has length 4) -> bits uint8 [n][bits_stride], the frame's
        info_bits(modulation, rate) information bits packed as reencode reads them: 16 SERVICE bits, the payload
        and its CRC-32 FCS, six tail bits and the pad, scrambled from `seed` (1..127) with the tail zeroed.
        length is the PSDU length with the FCS, 4..psdu_max_len (None: the longest); lengths int32 [n] and seeds
        uint8 [n] give every frame its own (a frame whose entry is out of range gets a row of zeros).  The strides
        default to max - 4 (length - 4 without lengths) and ceil(T / 8)."""
        nbytes, mx = (info_bits(modulation, rate) + 7) // 8, psdu_max_len(modulation, rate)
        L = mx if length is None else int(length)
        p = PsduPar(modulation, rate, L, int(seed), _addr(lengths), _addr(seeds))
        ps = payload_stride if payload_stride is not None else (mx if lengths is not None else L) - 4
        _check(_lib.wce_psdu_frame(self.handle, byref(p), _addr(payload), ps, n_frames, _addr(bits),
                                   bits_stride if bits_stride is not None else nbytes, stream), "wce_psdu_frame")

    def psdu_deframe(self, bits, n_frames, modulation, rate, length=None, lengths=None, psdu=None, seed=None,
                     fcs_ok=None, n_good=None, bits_stride=None, psdu_stride=None, stream=None):
        """wce_psdu_deframe on device arrays: bits uint8 [n][bits_stride] (viterbi_decode's packed rows, decoded
        with terminated=False) -> psdu uint8 [n][psdu_stride], the descrambled PSDU octets with their FCS
        (length of them, or lengths[n]; nothing beyond is written), seed uint8 [n], the scrambler state the
        first seven bits give (0: they are all zero, and the PSDU is written undescrambled), fcs_ok uint32 [n]
        (1: the CRC-32 over the PSDU leaves the residue) and n_good uint32 [1], to which the number of good
        frames is ADDED.  Each output is optional.  A frame whose lengths entry is out of range: fcs_ok 0, seed 0,
        no PSDU octet written.  The strides default to ceil(T / 8) and max (length without lengths)."""
        nbytes, mx = (info_bits(modulation, rate) + 7) // 8, psdu_max_len(modulation, rate)
        L = mx if length is None else int(length)
        p = PsduPar(modulation, rate, L, 0, _addr(lengths), None)
        o = PsduOut(_addr(psdu), psdu_stride if psdu_stride is not None else (mx if lengths is not None else L),
                    _addr(seed), _addr(fcs_ok), _addr(n_good))
        _check(_lib.wce_psdu_deframe(self.handle, byref(p), _addr(bits),
                                     bits_stride if bits_stride is not None else nbytes, n_frames, byref(o), stream),
               "wce_psdu_deframe")

    def psdu_frame_host(self, payloads, modulation, rate, seeds=93):
        """Convenience: host payloads, a list of byte rows (bytes or uint8 arrays, each 0..psdu_max_len - 4 long,
        their lengths free) or a 2-D uint8 array, and seeds (a scalar or [B]) -> bits uint8 [B][T], one framed
        information bit per entry (psdu_frame, unpacked)."""
        rows = [np.frombuffer(bytes(r), np.uint8) if isinstance(r, (bytes, bytearray)) else np.asarray(r, np.uint8)
                for r in payloads]
        B, T, mx = len(rows), info_bits(modulation, rate), psdu_max_len(modulation, rate)
        if any(r.ndim != 1 or r.size > mx - 4 for r in rows):
            raise ValueError(f"each payload must be a byte row of at most {mx - 4} octets")
        pay = np.zeros((B, mx - 4), np.uint8)
        for f, r in enumerate(rows):
            pay[f, :r.size] = r
        lengths = np.array([r.size + 4 for r in rows], np.int32)
        sd = np.broadcast_to(np.asarray(seeds, np.int64), (B,))
        if np.any(sd < 1) or np.any(sd > 127):
            raise ValueError("seeds must be 1..127")
        sd = np.ascontiguousarray(sd.astype(np.uint8))
        dbits = DeviceArray((B, (T + 7) // 8), np.uint8, zero=True)
        keep = (DeviceArray.from_numpy(pay), DeviceArray.from_numpy(lengths), DeviceArray.from_numpy(sd))
        self.psdu_frame(keep[0], B, modulation, rate, lengths=keep[1], seeds=keep[2], bits=dbits)
        synchronize()
        return np.unpackbits(dbits.numpy(), axis=1, bitorder="little")[:, :T]

    def psdu_deframe_host(self, bits, modulation, rate, lengths):
        """Convenience: host bits [B][T] (one information bit per entry, as decode_host returns them) and the PSDU
        lengths (a scalar or [B], FCS included) -> dict of host arrays: psdu uint8 [B][max] (row f holds
        lengths[f] octets, the rest 0), seed uint8 [B], fcs_ok uint32 [B] and n_good, their number (psdu_deframe)."""
        bits = np.asarray(bits, np.uint8)
        T, mx = info_bits(modulation, rate), psdu_max_len(modulation, rate)
        if bits.ndim != 2 or bits.shape[1] != T:
            raise ValueError("bits must be [B][T] with T = info_bits(modulation, rate)")
        B = bits.shape[0]
        ln = np.ascontiguousarray(np.broadcast_to(np.asarray(lengths), (B,)).astype(np.int32))
        dbits = DeviceArray.from_numpy(np.packbits(bits, axis=1, bitorder="little"))
        dlen = DeviceArray.from_numpy(ln)
        d = {"psdu": DeviceArray((B, mx), np.uint8, zero=True), "seed": DeviceArray((B,), np.uint8, zero=True),
             "fcs_ok": DeviceArray((B,), np.uint32, zero=True), "n_good": DeviceArray((1,), np.uint32, zero=True)}
        self.psdu_deframe(dbits, B, modulation, rate, lengths=dlen, **d)
        synchronize()
        res = {n: a.numpy() for n, a in d.items()}
        res["n_good"] = int(res["n_good"][0])
        return res

    def modulate(self, sym, n_frames, wave, n_blocks=NBLK, tx_pre=None, pre_stride=0, frame_stride=None,
                 block_stride=NSC, wave_stride=None, stream=None):
        """wce_modulate on device arrays: sym complex [n][n_blocks][block_stride] (53 bins a block, e.g. reencode's
        tx) and, with tx_pre, the preamble's 53 bins ([53] shared with pre_stride 0, or [n][pre_stride]) -> wave
        complex [n][wave_stride], the clean time-domain waveform: the 160-sample long training field (with
        tx_pre), then 80 samples a block, cyclic prefix first.  The inverse of front_end_preamble / _blocks.  The
        frame stride defaults to n_blocks block strides, the wave stride to the waveform's length."""
        S = (160 if tx_pre is not None else 0) + SAMPLES_PER_BLOCK * n_blocks
        _check(_lib.wce_modulate(self.handle, _addr(tx_pre), pre_stride, _addr(sym),
                                 frame_stride if frame_stride is not None else n_blocks * block_stride, block_stride,
                                 n_blocks, n_frames, _addr(wave), wave_stride if wave_stride is not None else S,
                                 stream), "wce_modulate")

    def short_field(self, wave, n_frames, amplitude=1.0, wave_stride=STF_LEN, stream=None):
        """wce_short_field on a device array: wave complex [n][wave_stride], whose first 160 samples of each row
        become 802.11a's short training field at `amplitude` (1: the mean sample power of a long field of unit
        bins, 52/4096).  A packet with a short field: this, then modulate from wave + 160 samples, then channel
        with wave_len 1520."""
        _check(_lib.wce_short_field(self.handle, amplitude, _addr(wave), wave_stride, n_frames, stream),
               "wce_short_field")

    def stf_amplitude(self):
        """the short field's amplitude that matches the context's tx preamble: the rms of its non-zero bins"""
        if self.tx_pre is None:
            raise ValueError("the context has no tx preamble")
        p = np.abs(np.asarray(self.tx_pre).ravel())
        return float(np.sqrt(np.mean(p[p != 0] ** 2)))

    @staticmethod
    def _channel_par(taps, n_taps, taps_stride, field, cfo, ow2, delay, seed, first_frame):
        return ChannelPar(_addr(taps), taps_stride, n_taps, int(bool(field)), _addr(cfo), _addr(ow2), _addr(delay),
                          seed, first_frame)

    def channel(self, wave, n_frames, wave_len, capture, capture_len, taps=None, n_taps=1, taps_stride=0, field=True,
                cfo=None, ow2=None, delay=None, seed=0x80211, first_frame=0, wave_stride=None, capture_stride=None,
                stream=None):
        """wce_channel on device arrays: wave complex [n][wave_stride] (modulate's) -> capture complex
        [n][capture_stride], raw capture windows of capture_len samples: the waveform through the frame's n_taps
        taps (complex [n_taps] shared with taps_stride 0, or [n][taps_stride]; None: one unit tap), turned by
        exp(2 pi i cfo[f] n) (cfo float64 [n], cycles per sample; n counts from the end of the field when `field`),
        placed delay[f] (int32 [n], any sign) samples into the window and clipped to it, plus CN(0, ow2[f])
        Gaussian noise (ow2 float64 [n]) drawn from (seed, first_frame + f, sample).  The input of front_end_sync."""
        p = self._channel_par(taps, n_taps, taps_stride, field, cfo, ow2, delay, seed, first_frame)
        _check(_lib.wce_channel(self.handle, _addr(wave), wave_stride if wave_stride is not None else wave_len,
                                wave_len, n_frames, byref(p), _addr(capture),
                                capture_stride if capture_stride is not None else capture_len, capture_len, stream),
               "wce_channel")

    def transmit(self, sym, n_frames, capture, capture_len, n_blocks=NBLK, tx_pre=None, pre_stride=0,
                 frame_stride=None, block_stride=NSC, taps=None, n_taps=1, taps_stride=0, cfo=None, ow2=None,
                 delay=None, seed=0x80211, first_frame=0, capture_stride=None, stream=None):
        """wce_transmit on device arrays: modulate and channel in one launch, the bits of the two calls in
        sequence; the clean waveform never goes through memory.  Arguments as theirs; the field is there with
        tx_pre."""
        p = self._channel_par(taps, n_taps, taps_stride, tx_pre is not None, cfo, ow2, delay, seed, first_frame)
        _check(_lib.wce_transmit(self.handle, _addr(tx_pre), pre_stride, _addr(sym),
                                 frame_stride if frame_stride is not None else n_blocks * block_stride, block_stride,
                                 n_blocks, n_frames, byref(p), _addr(capture),
                                 capture_stride if capture_stride is not None else capture_len, capture_len, stream),
               "wce_transmit")

    @staticmethod
    def _fading_par(knots, n_knots, knot_period, n_taps, knot_stride, knots_frame_stride, field, cfo, ow2, delay,
                    seed, first_frame):
        return FadingPar(_addr(knots), knots_frame_stride, knot_stride if knot_stride is not None else n_taps,
                         n_knots, knot_period, n_taps, int(bool(field)), _addr(cfo), _addr(ow2), _addr(delay), seed,
                         first_frame)

    def channel_tv(self, wave, n_frames, wave_len, capture, capture_len, knots, n_knots, knot_period=80, n_taps=1,
                   knot_stride=None, knots_frame_stride=0, field=True, cfo=None, ow2=None, delay=None, seed=0x80211,
                   first_frame=0, wave_stride=None, capture_stride=None, stream=None):
        """wce_channel_tv on device arrays: channel with taps that move within the packet.  knots complex
        [n][knots_frame_stride] (0: one trajectory [n_knots][knot_stride] shared by all frames), n_knots sets of
        n_taps taps knot_period samples apart, the first under the waveform's first sample; a tap is interpolated
        linearly between its knots, and the knots must reach past the last output: (n_knots - 1) knot_period >
        wave_len + n_taps - 2.  knot_stride defaults to n_taps.  Everything else as channel; constant knots give
        channel's bits."""
        p = self._fading_par(knots, n_knots, knot_period, n_taps, knot_stride, knots_frame_stride, field, cfo, ow2,
                             delay, seed, first_frame)
        _check(_lib.wce_channel_tv(self.handle, _addr(wave), wave_stride if wave_stride is not None else wave_len,
                                   wave_len, n_frames, byref(p), _addr(capture),
                                   capture_stride if capture_stride is not None else capture_len, capture_len,
                                   stream), "wce_channel_tv")

    def transmit_tv(self, sym, n_frames, capture, capture_len, knots, n_knots, knot_period=80, n_taps=1,
                    knot_stride=None, knots_frame_stride=0, n_blocks=NBLK, tx_pre=None, pre_stride=0,
                    frame_stride=None, block_stride=NSC, cfo=None, ow2=None, delay=None, seed=0x80211, first_frame=0,
                    capture_stride=None, stream=None):
        """wce_transmit_tv on device arrays: modulate and channel_tv in one launch, the bits of the two calls in
        sequence.  Arguments as transmit's and channel_tv's; a full packet at knot_period 80 takes 19 knots."""
        p = self._fading_par(knots, n_knots, knot_period, n_taps, knot_stride, knots_frame_stride,
                             tx_pre is not None, cfo, ow2, delay, seed, first_frame)
        _check(_lib.wce_transmit_tv(self.handle, _addr(tx_pre), pre_stride, _addr(sym),
                                    frame_stride if frame_stride is not None else n_blocks * block_stride,
                                    block_stride, n_blocks, n_frames, byref(p), _addr(capture),
                                    capture_stride if capture_stride is not None else capture_len, capture_len,
                                    stream), "wce_transmit_tv")

    def _transmit_device(self, dsym, B, n_blocks, dpre, pre_stride, taps, cfo, ow2, delay, capture_len, seed,
                         first_frame, fused, knot_period=None, stf=False):
        """transmit_host's device half: symbols (and the preamble) on the device, the channel's per-frame
        parameters on the host -> (capture DeviceArray [B][capture_len], what the queued calls read until the
        caller synchronises).  Taps with a knot axis ([B][K][n_taps], or [K][n_taps] with knot_period given) go
        through the time-varying calls.  stf: the short field in front (short_field, modulate 160 samples in,
        channel over the 1,520 samples; never fused)."""
        if stf and dpre is None:
            raise ValueError("stf needs a tx preamble: the short field goes in front of the long one")
        dtaps, n_taps, ts = None, 1, 0
        tv = taps is not None and (np.ndim(taps) == 3 or (np.ndim(taps) == 2 and knot_period is not None))
        if tv:
            taps = _as_c128(taps)
            if taps.ndim == 3 and taps.shape[0] != B:
                raise ValueError("taps with knots must be [K][n_taps] or [B][K][n_taps] complex")
            n_knots, n_taps = taps.shape[-2], taps.shape[-1]
            kfs = n_knots * n_taps if taps.ndim == 3 else 0
            dtaps = DeviceArray.from_numpy(taps)
        elif taps is not None:
            taps = _as_c128(taps)
            if taps.ndim not in (1, 2) or (taps.ndim == 2 and taps.shape[0] != B):
                raise ValueError("taps must be [n_taps] or [B][n_taps] complex")
            n_taps, ts = taps.shape[-1], (taps.shape[1] if taps.ndim == 2 else 0)
            dtaps = DeviceArray.from_numpy(taps)

        def per_frame(x, dtype):   # a scalar or [B] -> a device array [B]
            if x is None:
                return None
            return DeviceArray.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=dtype), (B,))))
        dcfo, dow2, ddelay = per_frame(cfo, np.float64), per_frame(ow2, np.float64), per_frame(delay, np.int32)
        S = (160 if dpre is not None else 0) + SAMPLES_PER_BLOCK * n_blocks
        dcap = DeviceArray((B, capture_len), zero=True)
        keep = [dtaps, dcfo, dow2, ddelay]

        def wave():   # the clean waveform, unfused: [short field,] long field, blocks
            W = S + (STF_LEN if stf else 0)
            dwave = DeviceArray((B, W), zero=True)
            keep.append(dwave)
            if stf:
                self.short_field(dwave, B, self.stf_amplitude(), W)
                self.modulate(dsym, B, dwave.addr + STF_LEN * 16, n_blocks, dpre, pre_stride, wave_stride=W)
            else:
                self.modulate(dsym, B, dwave, n_blocks, dpre, pre_stride)
            return dwave, W
        fused = fused and not stf
        if tv:
            P = 80 if knot_period is None else int(knot_period)
            kn = dict(knots=dtaps, n_knots=n_knots, knot_period=P, n_taps=n_taps, knot_stride=n_taps,
                      knots_frame_stride=kfs, cfo=dcfo, ow2=dow2, delay=ddelay, seed=seed, first_frame=first_frame)
            if fused:
                self.transmit_tv(dsym, B, dcap, capture_len, n_blocks=n_blocks, tx_pre=dpre, pre_stride=pre_stride,
                                 **kn)
            else:
                dwave, W = wave()
                self.channel_tv(dwave, B, W, dcap, capture_len, field=dpre is not None, **kn)
        elif fused:
            self.transmit(dsym, B, dcap, capture_len, n_blocks, dpre, pre_stride, taps=dtaps, n_taps=n_taps,
                          taps_stride=ts, cfo=dcfo, ow2=dow2, delay=ddelay, seed=seed, first_frame=first_frame)
        else:
            dwave, W = wave()
            self.channel(dwave, B, W, dcap, capture_len, dtaps, n_taps, ts, dpre is not None, dcfo, dow2, ddelay,
                         seed, first_frame)
        return dcap, keep

    def transmit_host(self, sym, tx_pre=None, taps=None, cfo=None, ow2=None, delay=None, capture_len=None,
                      seed=0x80211, first_frame=0, fused=True, stf=False, knot_period=None):
        """Convenience: host symbols sym [B][n_blocks][53] (n_blocks 0..15) and, optionally, the preamble's 53
        bins tx_pre ([53] shared, or [B][53]) -> raw capture windows [B][capture_len] on the host.  taps [n_taps]
        or [B][n_taps] complex (None: a unit tap); cfo (cycles per sample), ow2 (noise variance per complex
        sample) and delay (int, any sign): a scalar or [B], None = 0.  capture_len defaults to the waveform's
        length plus the taps' tail.  fused: one transmit launch, else modulate then channel -- the same bits.
        Taps that move within the packet (transmit_tv; fading_taps draws them): [B][K][n_taps], K knots
        knot_period samples apart (None: 80, a knot per block boundary, K = 19 for a full packet), or one shared
        trajectory [K][n_taps], which needs knot_period given: without it 2-D taps are [B][n_taps].
        stf: 802.11a's short training field (short_field, at the rms of the context's non-zero tx preamble bins)
        goes in front of the long one, which tx_pre must then provide: 160 samples more, built unfused; the
        channel's time origin stays at the end of the first 160 samples."""
        sym = _as_c128(sym)
        if sym.ndim != 3 or sym.shape[2] != NSC or sym.shape[1] > NBLK:
            raise ValueError("sym must be [B][n_blocks <= 15][53] complex")
        B, n_blocks = sym.shape[0], sym.shape[1]
        dpre, ps = None, 0
        if tx_pre is not None:
            tx_pre = _as_c128(tx_pre)
            if tx_pre.shape not in ((NSC,), (B, NSC)):
                raise ValueError("tx_pre must be [53] or [B][53] complex")
            dpre, ps = DeviceArray.from_numpy(tx_pre), (NSC if tx_pre.ndim == 2 else 0)
        dsym = DeviceArray.from_numpy(sym) if n_blocks else None
        if capture_len is None:
            capture_len = (160 if dpre is not None else 0) + SAMPLES_PER_BLOCK * n_blocks + \
                (np.shape(taps)[-1] if taps is not None else 1) - 1 + (STF_LEN if stf else 0)
        dcap, keep = self._transmit_device(dsym, B, n_blocks, dpre, ps, taps, cfo, ow2, delay, int(capture_len), seed,
                                           first_frame, fused, knot_period, stf)
        synchronize()
        return dcap.numpy()

    def link_host(self, modulation, rate, snr_db, n_frames, sources=(LT_LS, PS_LINEAR, PS_MMSE), taps=None, cfo=None,
                  delay=None, capture_len=1488, threshold=0.25, backoff=0, seed=0x80211, dd_iterations=0,
                  scale=8.8753, stf=False, stf_threshold=0.25, psdu_len=None, knot_period=80, tracker=None):
        """The experiment WiFi_RX.m:4-9 announces (SNR, channel_model, FO), for a batch, scored in coded bit
        errors: n_frames packets of random information bits (drawn on the host from `seed`, the last six 0) are
        re-encoded to symbols with 802.11's pilots, transmitted behind the context's tx preamble through `taps`
        ([n_taps] or [B][n_taps], None: a unit tap; pdp_taps draws them), a carrier offset cfo and a delay (scalar
        or [B]) with Gaussian noise at snr_db (scalar or [B]) into capture windows of capture_len samples, and
        received: front_end_sync, the field with its own offset estimate, the blocks, estimate, and per source
        (estimator bits) demodulate (tracked; blended with lt_ls for every source but LT_LS), soft_demap and
        viterbi_decode against the sent bits.  Everything between the bits going up and the counts coming down
        is queued on one stream; the capture never visits the host.
        snr_db is nominal: ow2 = (52 scale^2 / 4096) / 10^(snr_db / 10), the mean power of a sample of a frame
        of unit-mean-energy constellation points over the noise variance, for taps with sum |h|^2 = 1.  PS_MMSE
        takes each frame's ow2 from it on a TEXTBOOK context (with the frame's own preamble as covariance), the
        context's ow2 and covariance otherwise.
        dd_iterations n > 0: n decision-directed rounds behind each source's decoder; its count is the last
        round's.
        taps [B][K][n_taps] (fading_taps draws them): a channel that moves within the packet, K knots
        knot_period samples apart, through transmit_tv.  tracker (mu, beta): each source's estimate additionally
        starts a track_demodulate (no blend, phase tracking on) on the same capture, followed by
        soft_demap_blocks on its h_blocks and viterbi_decode; not together with dd_iterations.
        stf: the packet carries 802.11a's short training field in front of the long one (1,520 samples; the
        waveform is built unfused, and 3-D taps need knots that cover them) and the receiver runs
        front_end_sync_stf (thresholds stf_threshold and threshold), which detects at any carrier offset and
        estimates |cfo| < 1/32 cycles per sample, then the field and the blocks at its start and offset; the
        result gains "metric_stf", and "metric" is the long field's.  capture_len must hold the packet,
        1520 + n_taps - 1 + the largest delay samples (1,648 is a window with room for 128 more), else ValueError.
        -> {source: nbiterr uint32 [B]} plus "start" int32 [B] (-1: not detected; its counts are those of an
        all-zero decode), "metric" [B], "cfo" [B] (the estimate), "ow2" [B] and "bits" uint8 [B][T]; with
        tracker, "tracked": {source: nbiterr uint32 [B]} of the tracked runs.
        psdu_len L (4..psdu_max_len): the packets carry real PSDUs and are judged as a receiver in the field
        judges them.  Payload octets rng.integers(0, 256, (B, L - 4)) and scrambler seeds rng.integers(1, 128, B)
        are drawn from `seed` instead of the bits, framed on the device (psdu_frame) and fed to reencode; every
        decode runs unterminated (the tail is not at the end of the field) against the framed bits, and
        psdu_deframe is queued behind each source's last decoder and each tracked one.  The result gains
        "fcs_ok" {source: uint32 [B]}, "psdu_rx" {source: uint8 [B][L]}, "seed_rx" {source: uint8 [B]}, "bits_rx"
        {source: uint8 [B][T]} (the decoded rows), "payload" uint8 [B][L - 4], "seeds" uint8 [B] and, with tracker,
        "tracked_fcs_ok" {source: uint32 [B]}; "bits" is the framed bits."""
        runs, f, ow2, bits, framed, _ = self._link(
            "link_host", modulation, rate, snr_db, n_frames, sources, taps, cfo, delay, capture_len, threshold,
            backoff, seed, dd_iterations, scale, stf, stf_threshold, psdu_len, knot_period, tracker)
        T = bits.shape[1]
        runs = {s: r[0] for s, r in runs.items()}   # one branch, alone
        res = {s: last["nbiterr"].numpy() for s, (last, tdec, _) in runs.items()}
        if tracker is not None:
            res["tracked"] = {s: tdec["nbiterr"].numpy() for s, (last, tdec, _) in runs.items()}
        res.update(start=f["start"].numpy(), metric=f["metric"].numpy(), cfo=f["cfo"].numpy(), ow2=ow2[0], bits=bits)
        if psdu_len is not None:
            rx = {s: last["_psdu"] for s, (last, tdec, _) in runs.items()}
            res.update(payload=framed[0], seeds=framed[1], fcs_ok={s: d["fcs_ok"].numpy() for s, d in rx.items()},
                       psdu_rx={s: d["psdu"].numpy() for s, d in rx.items()},
                       seed_rx={s: d["seed"].numpy() for s, d in rx.items()},
                       bits_rx={s: np.unpackbits(last["bits"].numpy(), axis=1, bitorder="little")[:, :T]
                                for s, (last, tdec, _) in runs.items()})
            if tracker is not None:
                res["tracked_fcs_ok"] = {s: tdec["_psdu"]["fcs_ok"].numpy() for s, (last, tdec, _) in runs.items()}
        if stf:
            res["metric_stf"] = f["metric_stf"].numpy()
        return res

    def _link(self, who, modulation, rate, snr_db, n_frames, sources, taps, cfo, delay, capture_len, threshold,
              backoff, seed, dd_iterations, scale, stf, stf_threshold, psdu_len, knot_period, tracker, n_rx=None,
              branch_loss_db=None, share_sync=False, weighted=False):
        """link_host's and link_mrc_host's body (`who` names the caller in a refusal): A branches of B packets,
        queued and synchronised once.  n_rx None: link_host -- one branch through `taps`, received from the
        transmitter's own capture, nothing shared, copied or combined.  n_rx A: link_mrc_host -- `taps` holds a
        set per branch, the captures go into one [A B][L] array, and per source the branches are also combined
        and the B combined frames go through the same chain.
        -> (runs {source: [alone] or [alone, combined]}, each what _chain_device returns; _capture_front's dict;
        ow2 [A][B] as transmitted; bits [B][T] as sent; (payload, seeds) or None; the capture on the device)"""
        mrc = n_rx is not None
        A, B, T = int(n_rx) if mrc else 1, int(n_frames), info_bits(modulation, rate)
        if psdu_len is not None and not 4 <= int(psdu_len) <= psdu_max_len(modulation, rate):
            raise ValueError(f"psdu_len must be 4..{psdu_max_len(modulation, rate)} octets")
        if mrc and not 1 <= A <= COMBINE_MAX_BRANCHES:
            raise ValueError("n_rx must be 1..8")
        if tracker is not None and dd_iterations:
            raise ValueError("tracker with dd_iterations > 0 (decoder-in-the-loop tracking) is not built")
        if tracker is not None:
            mu, beta = tracker   # not a pair: refused here, before the device
        if self.tx_pre is None:
            raise ValueError(f"{who} needs a context built from a tx preamble")
        names = {bit: n for n, bit in _ESTIMATORS}
        sources = tuple(sources)
        if not sources or any(s not in names for s in sources):
            raise ValueError("sources must be estimator bits")
        loss = np.zeros(A)
        if mrc:
            taps = _as_c128(taps)
            if taps.ndim not in (2, 3, 4) or taps.shape[0] != A or (taps.ndim >= 3 and taps.shape[1] != B):
                raise ValueError("taps must be [A][n_taps], [A][B][n_taps] or [A][B][K][n_taps] complex")
            if branch_loss_db is not None:
                loss = np.asarray(branch_loss_db, np.float64)
            if loss.shape != (A,):
                raise ValueError("branch_loss_db must be [A]")
        if stf:
            need = 1520 + (np.shape(taps)[-1] if taps is not None else 1) - 1 + \
                (int(np.max(delay)) if delay is not None else 0)
            if capture_len < need:
                raise ValueError(f"capture_len {capture_len} cannot hold a packet with a short field: {need} samples")
        branch = taps if mrc else [taps]
        N, L = A * B, int(capture_len)
        rng = np.random.default_rng(seed)
        if psdu_len is None:
            bits, framed = rng.integers(0, 2, (B, T), dtype=np.uint8), None
            bits[:, T - 6:] = 0
            ref = np.tile(bits, (A, 1))
            dbits = DeviceArray.from_numpy(np.packbits(ref, axis=1, bitorder="little"))
        else:   # the references stay on the device: the first B rows of dbits are the packets themselves
            dbits, framed = self._psdu_draw(rng, B, A, modulation, rate, int(psdu_len))
            ref = bits = dbits
        ow2 = np.ascontiguousarray(np.broadcast_to(
            (52.0 * scale * scale / 4096.0) / 10.0 ** (np.asarray(snr_db, np.float64) / 10.0), (B,))[None] *
            10.0 ** (loss / 10.0)[:, None])
        dtx = DeviceArray((N, NBLK, NSC), zero=True)   # the same symbols once per branch: frame a B + f is packet f
        dpre = DeviceArray.from_numpy(self.tx_pre)
        dfield = DeviceArray((160,), zero=True)   # the clean field: its samples 32..95 are one period, sync's ltf
        self.reencode(dbits, N, modulation, rate, scale, tx=dtx)
        self.modulate(None, 1, dfield, 0, dpre)
        sent = [self._transmit_device(dtx, B, NBLK, dpre, 0, branch[a], cfo, ow2[a], delay, L, seed, a * B, True,
                                      knot_period if np.ndim(branch[a]) == 3 else None, stf) for a in range(A)]
        if mrc:
            dcap, dow2 = DeviceArray((N, L), zero=True), DeviceArray.from_numpy(ow2)
            for a, (cap_a, _) in enumerate(sent):
                _check(_lib.wce_memcpy_dtod(c_void_p(dcap.addr + a * B * L * 16), cap_a.ptr, B * L * 16, None),
                       "wce_memcpy_dtod")
        else:   # the transmitter's own capture, and its ow2 on the device
            dcap, dow2 = sent[0][0], sent[0][1][2]
        f = self._capture_front(dcap, N, L, dfield.addr + 32 * 16, threshold, backoff, stf, stf_threshold,
                                share=(B, A) if share_sync and A > 1 else None)
        mask = LT_LS
        for s in sources:
            mask |= s
        outs = {n: DeviceArray((N, NSC), zero=True) for n, bit in _ESTIMATORS if mask & bit}
        o = Outputs(*[(outs[n].addr if n in outs else None) for n, _ in _ESTIMATORS], None, NSC, NBLK * NSC, NSC,
                    PS_LINEAR, 0)
        fr = self.frames(dtx, f["rx"], N, rx_pre=f["rx_pre"], tx_pre=dpre)
        if mask & PS_MMSE and self.mode == MMSE_TEXTBOOK:
            self.estimate(fr, o, mask | FRAME_COV, ow2=dow2)
        else:
            self.estimate(fr, o, mask)
        chain = (modulation, rate, scale, psdu_len is None, int(dd_iterations), tracker, psdu_len)
        runs, keep = {}, []
        for s in sources:
            h = outs[names[s]]
            runs[s] = [self._chain_device(fr, N, h, None if s == LT_LS else outs["lt_ls"], ref, *chain)]
            if mrc:
                drxc, dhc = DeviceArray((B, NBLK, NSC), zero=True), DeviceArray((B, NSC), zero=True)
                self.combine(f["rx"], h, B, A, f["ow2"] if weighted else None, drxc, dhc)
                runs[s].append(self._chain_device(self.frames(dtx, drxc, B), B, dhc, None, bits, *chain))
                keep += [drxc, dhc]
        synchronize()
        if psdu_len is not None:
            bits = np.unpackbits(dbits.rows(0, B), axis=1, bitorder="little")[:, :T]
        return runs, f, ow2, bits, framed, dcap

    def _capture_front(self, dcap, N, L, ltf, threshold, backoff, stf, stf_threshold, cfo=True, sample_offset=0,
                       share=None):
        """queue the front end on the device capture windows dcap [N][L], each call reading what the one before
        wrote: front_end_sync against ltf (front_end_sync_stf with stf, which also gives the offset), the field
        and the blocks at its start.  cfo False (and no stf): no offset is estimated or removed.  share (B, A):
        the windows are A branches of B packets and sync_share gives every branch the best one's start and
        offset -- without stf the start first, then the fields for the offsets, then the offset, and the fields
        again with it.  -> name -> DeviceArray (read them after a synchronize): start, metric, cfo (None without
        one), ow2 (the estimate), rx, rx_pre and, with stf, metric_stf"""
        f = {"start": DeviceArray((N,), np.int32, zero=True), "metric": DeviceArray((N,), np.float64, zero=True),
             "ow2": DeviceArray((N,), np.float64, zero=True),
             "cfo": DeviceArray((N,), np.float64, zero=True) if cfo or stf else None,
             "rx": DeviceArray((N, NBLK, NSC), zero=True), "rx_pre": DeviceArray((N, NSC), zero=True)}
        at = dict(cfo=f["cfo"], start=f["start"])
        if stf:
            f["metric_stf"] = DeviceArray((N,), np.float64, zero=True)
            self.front_end_sync_stf(dcap, N, L, ltf, stf_threshold, threshold, backoff, f["start"], f["cfo"],
                                    f["metric_stf"], f["metric"])
            if share:
                self.sync_share(f["metric"], *share, f["start"], f["cfo"])
        else:
            self.front_end_sync(dcap, N, L, ltf, threshold, backoff, f["start"], f["metric"])
            if share:   # one oscillator: the best branch's offset for all, and the fields again with it
                self.sync_share(f["metric"], *share, f["start"], None)
                self.front_end_preamble(dcap, N, L, f["rx_pre"], f["ow2"], **at)
                self.sync_share(f["metric"], *share, None, f["cfo"])
        self.front_end_preamble(dcap, N, L, f["rx_pre"], f["ow2"], estimate_cfo=not (stf or share), **at)
        self.front_end_blocks(dcap, N, NBLK, f["rx"], sample_offset=sample_offset, capture_len=L, **at)
        return f

    def _chain_device(self, frames, n, h, hlt, ref, modulation, rate, scale, terminated, dd_rounds, tracker, psdu_len):
        """queue one source's receive chain on n frames: demodulate (tracked, against tx) with h and h_lt,
        soft_demap and viterbi_decode against ref, then dd_rounds decision-directed rounds; with tracker (mu,
        beta), beside it, track_demodulate from h, soft_demap_blocks and viterbi_decode; with psdu_len,
        psdu_deframe behind each last decoder, its dict under "_psdu".  -> (the static chain's last decode, the
        tracked one or None, what else the queued calls read), name -> DeviceArray (read after a synchronize)"""
        dem = self._demod_device(frames, n, h, hlt, modulation, scale, True, True)
        dec = self._decode_device(dem["eq"], h, hlt, n, modulation, rate, scale, terminated, ref)
        last = self._dd_device(frames, n, dec["bits"], dem["theta"], modulation, rate, scale, terminated, dec["_ref"],
                               dd_rounds) if dd_rounds else dec
        trk = tdec = None
        if tracker is not None:
            trk = self._track_device(frames, n, h, tracker[0], tracker[1], modulation, scale, True, True)
            tdec = self._decode_device(trk["eq"], None, None, n, modulation, rate, scale, terminated, ref,
                                       h_blocks=trk["h_blocks"])
        if psdu_len is not None:
            last = dict(last, _psdu=self._psdu_device(last["bits"], n, modulation, rate, int(psdu_len)))
            if tdec is not None:
                tdec = dict(tdec, _psdu=self._psdu_device(tdec["bits"], n, modulation, rate, int(psdu_len)))
        return last, tdec, (dem, dec, trk)

    def _psdu_draw(self, rng, B, copies, modulation, rate, L):
        """link_host's packets with PSDUs: payload octets [B][L - 4] and scrambler seeds [B] from rng, framed on
        the device `copies` times over (frame a B + f is packet f) -> (packed bits DeviceArray [copies B][ceil(T / 8)],
        (payload, seeds))"""
        payload = rng.integers(0, 256, (B, L - 4)).astype(np.uint8)
        seeds = rng.integers(1, 128, B).astype(np.uint8)
        dbits = DeviceArray((copies * B, (info_bits(modulation, rate) + 7) // 8), np.uint8, zero=True)
        dpay = DeviceArray.from_numpy(np.tile(payload, (copies, 1))) if L > 4 else None
        dseeds = DeviceArray.from_numpy(np.tile(seeds, copies))
        self.psdu_frame(dpay, copies * B, modulation, rate, length=L, seeds=dseeds, bits=dbits)
        synchronize()   # the payload and the seeds are free to go
        return dbits, (payload, seeds)

    def _psdu_device(self, dbits, n, modulation, rate, L):
        """queue psdu_deframe behind a decoder's packed bits -> name -> DeviceArray (read after a synchronize)"""
        d = {"psdu": DeviceArray((n, L), np.uint8, zero=True), "seed": DeviceArray((n,), np.uint8, zero=True),
             "fcs_ok": DeviceArray((n,), np.uint32, zero=True)}
        self.psdu_deframe(dbits, n, modulation, rate, length=L, **d)
        return d

    def combine(self, rx, h, n_frames, n_branches, ow2=None, out_rx=None, out_h=None, rx_branch_stride=None,
                rx_frame_stride=None, rx_block_stride=NSC, h_branch_stride=None, h_stride=NSC,
                ow2_branch_stride=None, out_frame_stride=None, out_block_stride=NSC, out_h_stride=NSC, stream=None):
        """wce_combine on device arrays: maximal-ratio combining of n_branches antenna branches of n_frames
        packets.  rx complex [A][n][15][53], h complex [A][n][53] (any estimate) and, optionally, ow2 float64
        [A][n] (each branch's noise variance: the weights become 1 / ow2 and the combined noise has unit variance;
        None: unit weights) -> out_rx complex [n][15][53] and out_h complex [n][53] (real: sqrt of the summed
        weighted |h|^2), each optional, laid out as every later call of the chain reads them.  A branch with a
        non-finite h row or an ow2 that is not finite and positive is left out, bit for bit; a packet with none
        left gets NaN rows.  The strides default to dense branch-major arrays (frame strides 15 block strides,
        branch strides n frame strides); any layout whose branches do not overlap is taken."""
        rfs = rx_frame_stride if rx_frame_stride is not None else NBLK * rx_block_stride
        p = CombinePar(_addr(rx), rx_branch_stride if rx_branch_stride is not None else n_frames * rfs, rfs,
                       rx_block_stride, _addr(h),
                       h_branch_stride if h_branch_stride is not None else n_frames * h_stride, h_stride, _addr(ow2),
                       ow2_branch_stride if ow2_branch_stride is not None else n_frames, n_branches)
        o = CombineOut(_addr(out_rx), out_frame_stride if out_frame_stride is not None else NBLK * out_block_stride,
                       out_block_stride, _addr(out_h), out_h_stride)
        _check(_lib.wce_combine(self.handle, byref(p), n_frames, byref(o), stream), "wce_combine")

    def sync_share(self, metric, n_packets, n_branches, start=None, cfo=None, branch_stride=None, stream=None):
        """wce_sync_share on device arrays [A][branch_stride]: the antennas of a radio share one oscillator and one
        packet arrival, so every branch of packet p takes the start (int32, front_end_sync's) and the offset cfo
        (float64) of the branch that detected it with the largest metric (float64; the lowest branch on a tie), in
        place.  A branch is live with start >= 0 and a finite metric; a packet with no live branch is left as it
        is.  start None: the offset alone is shared (live: a finite metric); cfo None: the start alone."""
        _check(_lib.wce_sync_share(self.handle, n_branches, branch_stride if branch_stride is not None else n_packets,
                                   n_packets, _addr(metric), _addr(start), _addr(cfo), stream), "wce_sync_share")

    def combine_host(self, rx, h, ow2=None):
        """Convenience: host branches rx [A][B][15][53], estimates h [A][B][53] and, optionally, noise variances
        ow2 [A][B] -> dict of host arrays rx [B][15][53] and h [B][53] (combine)."""
        rx, h = _as_c128(rx), _as_c128(h)
        if rx.ndim != 4 or rx.shape[2:] != (NBLK, NSC):
            raise ValueError("rx must be [A][B][15][53] complex")
        A, B = rx.shape[:2]
        if h.shape != (A, B, NSC):
            raise ValueError("h must be [A][B][53] complex")
        dow2 = None
        if ow2 is not None:
            ow2 = np.ascontiguousarray(ow2, np.float64)
            if ow2.shape != (A, B):
                raise ValueError("ow2 must be [A][B]")
            dow2 = DeviceArray.from_numpy(ow2)
        drx, dh = DeviceArray.from_numpy(rx), DeviceArray.from_numpy(h)
        d = {"rx": DeviceArray((B, NBLK, NSC), zero=True), "h": DeviceArray((B, NSC), zero=True)}
        self.combine(drx, dh, B, A, dow2, d["rx"], d["h"])
        synchronize()
        return {n: a.numpy() for n, a in d.items()}

    def link_mrc_host(self, modulation, rate, snr_db, n_frames, n_rx, taps, sources=(LT_LS, PS_LINEAR, PS_MMSE),
                      branch_loss_db=None, share_sync=True, weighted=True, cfo=None, delay=None, capture_len=1488,
                      threshold=0.25, backoff=0, seed=0x80211, dd_iterations=0, scale=8.8753, stf=False,
                      stf_threshold=0.25, knot_period=80, tracker=None, keep_capture=False, psdu_len=None):
        """link_host behind n_rx receive antennas: n_frames packets of random information bits (link_host's draw
        from `seed`) are re-encoded once and transmitted once per branch on the same symbols, through that
        branch's taps ([A][n_taps], or [A][B][n_taps]; with a knot axis, [A][B][K][n_taps], through transmit_tv)
        with a shared carrier offset cfo and delay and the branch's own noise (first_frame = a B: nominal snr_db
        as link_host, less branch_loss_db[a] dB, None: 0).  The receiver runs over all A B windows at once:
        front_end_sync (front_end_sync_stf with stf), sync_share (share_sync: a branch in a fade takes the start
        and the offset of the one that detected best), the _at front end, estimate, and per source (estimator
        bits) combine -- weighted by each branch's estimated noise variance, the front end's ow2 (weighted), or
        by 1 -- then demodulate (tracked phase, no blend), soft_demap and viterbi_decode on the combined stream;
        dd_iterations and tracker (mu, beta) as link_host, on the combined stream.  Each branch alone goes through
        link_host's own chain beside it.  Only bits go up and only error counts come down.
        -> {source: {"combined": nbiterr uint32 [B], "branch": nbiterr uint32 [A][B]}}; with tracker, "tracked":
        the same per source for the tracked runs; plus "start" int32, "metric", "cfo", "ow2" (the transmitter's)
        and "ow2_est" (the front end's), each [A][B], after sharing, and "bits" uint8 [B][T]; with stf,
        "metric_stf"; with keep_capture, "capture" complex [A][B][capture_len].  n_rx = 1 gives link_host's
        counts as branch 0.
        psdu_len L: as link_host -- the same draws, every branch sends the same framed bits, the decodes run
        unterminated and psdu_deframe follows each chain's last decoder.  The result gains "fcs_ok" {source:
        {"combined": uint32 [B], "branch": uint32 [A][B]}}, "psdu_rx" {source: uint8 [B][L]} (the combined
        chain's), "payload", "seeds" and, with tracker, "tracked_fcs_ok" like "fcs_ok"."""
        runs, f, ow2, bits, framed, dcap = self._link(
            "link_mrc_host", modulation, rate, snr_db, n_frames, sources, taps, cfo, delay, capture_len, threshold,
            backoff, seed, dd_iterations, scale, stf, stf_threshold, psdu_len, knot_period, tracker, n_rx,
            branch_loss_db, share_sync, weighted)
        A, B = ow2.shape

        def both(i, get):   # chain i (0: static or decision-directed, 1: tracked) of every source, combined and alone
            return {s: {"combined": get(comb[i]).numpy(), "branch": get(alone[i]).numpy().reshape(A, B)}
                    for s, (alone, comb) in runs.items()}
        res = both(0, lambda d: d["nbiterr"])
        if tracker is not None:
            res["tracked"] = both(1, lambda d: d["nbiterr"])
        if psdu_len is not None:
            res.update(fcs_ok=both(0, lambda d: d["_psdu"]["fcs_ok"]), payload=framed[0], seeds=framed[1],
                       psdu_rx={s: comb[0]["_psdu"]["psdu"].numpy() for s, (alone, comb) in runs.items()})
            if tracker is not None:
                res["tracked_fcs_ok"] = both(1, lambda d: d["_psdu"]["fcs_ok"])
        res.update({n: f[n].numpy().reshape(A, B) for n in ("start", "metric", "cfo")}, ow2=ow2,
                   ow2_est=f["ow2"].numpy().reshape(A, B), bits=bits)
        if stf:
            res["metric_stf"] = f["metric_stf"].numpy().reshape(A, B)
        if keep_capture:
            res["capture"] = dcap.numpy().reshape(A, B, -1)
        return res

    def _dd_device(self, fr, B, dbits, dtheta, modulation, rate, scale, terminated, dref, rounds):
        """queue `rounds` decision-directed passes behind a decode, on the same (null) stream with no host read:
        reencode(bits, theta -> h_dd) -> demodulate(h = h_dd, no blend, tracked) -> soft_demap -> viterbi_decode,
        each round on the bits and the block phases of the one before.  fr: the frames (rx, and tx for the
        pilots); dref: packed reference bits on the device or None.  -> name -> DeviceArray of the last round
        (h_dd, bits, nbiterr with dref; read them after a synchronize)"""
        T = info_bits(modulation, rate)
        d = {}
        for _ in range(rounds):
            d = {"h_dd": DeviceArray((B, NSC), zero=True), "bits": DeviceArray((B, (T + 7) // 8), np.uint8, zero=True),
                 "_keep": (dbits, dtheta, d)}   # read by the queued calls until the caller synchronises
            eq, theta = DeviceArray((B, NBLK, NSC), zero=True), DeviceArray((B, NBLK), np.float64, zero=True)
            llr = DeviceArray((B, NBLK, 48 * modulation), np.float32, zero=True)
            if dref is not None:
                d["nbiterr"] = DeviceArray((B,), np.uint32, zero=True)
            self.reencode(dbits, B, modulation, rate, scale, theta=dtheta, frames=fr, h=d["h_dd"])
            self.demodulate(fr, d["h_dd"], None, NSC, modulation, scale, True, True, eq=eq, theta=theta)
            self.soft_demap(eq, d["h_dd"], B, None, NSC, modulation, scale, llr)
            self.viterbi_decode(llr, B, modulation, rate, terminated, d["bits"], ref_bits=dref,
                                nbiterr=d.get("nbiterr"))
            d["_keep"] += (eq, llr, theta)
            dbits, dtheta = d["bits"], theta
        return d

    @staticmethod
    def _dd_result(d, modulation, rate):
        """-> (h_dd, decode_dd) of _dd_device's dict, on the host"""
        dd = {n: d[n].numpy() for n in ("bits", "nbiterr") if n in d}
        dd["bits"] = np.unpackbits(dd["bits"], axis=1, bitorder="little")[:, :info_bits(modulation, rate)]
        return d["h_dd"].numpy(), dd

    def _decode_device(self, deq, dh, dhlt, B, modulation, rate, scale, terminated, ref_bits, h_blocks=None):
        """queue soft_demap and viterbi_decode on dense device arrays (eq [B][15][53], h and h_lt [B][53]; or, with
        h_blocks [B][15][53], soft_demap_blocks and neither h nor h_lt);
        -> name -> DeviceArray (read them after a synchronize, through _decode_result)"""
        T = info_bits(modulation, rate)
        d = {"llr": DeviceArray((B, NBLK, 48 * modulation), np.float32, zero=True),
             "bits": DeviceArray((B, (T + 7) // 8), np.uint8, zero=True)}
        dref = None
        if isinstance(ref_bits, DeviceArray):   # packed rows [>= B][ceil(T / 8)] already there
            dref = ref_bits
            d["nbiterr"] = DeviceArray((B,), np.uint32, zero=True)
        elif ref_bits is not None:
            ref = np.asarray(ref_bits, np.uint8)
            if ref.shape != (B, T):
                raise ValueError("ref_bits must be [B][T] with T = info_bits(modulation, rate)")
            dref = DeviceArray.from_numpy(np.packbits(ref, axis=1, bitorder="little"))
            d["nbiterr"] = DeviceArray((B,), np.uint32, zero=True)
        if h_blocks is not None:
            self.soft_demap_blocks(deq, h_blocks, B, modulation, scale, d["llr"])
        else:
            self.soft_demap(deq, dh, B, dhlt, NSC, modulation, scale, d["llr"])
        self.viterbi_decode(d["llr"], B, modulation, rate, terminated, d["bits"], ref_bits=dref,
                            nbiterr=d.get("nbiterr"))
        d["_ref"] = dref   # read by the queued decoder until the caller synchronises
        return d

    @staticmethod
    def _decode_result(d, modulation, rate):
        res = {n: a.numpy() for n, a in d.items() if n != "_ref"}
        res["bits"] = np.unpackbits(res["bits"], axis=1, bitorder="little")[:, :info_bits(modulation, rate)]
        return res

    def decode_host(self, eq, h, h_lt=None, modulation=MOD_BPSK, rate=RATE_1_2, scale=8.8753, terminated=True,
                    ref_bits=None, dd_iterations=0, rx=None, tx_pilots=None):
        """Convenience: host equalized symbols eq [B][15][53] (demodulate_host's) and estimates h (and h_lt)
        [B][53] -> dict of host arrays: llr float32 [B][15][48 * modulation] (soft_demap), bits uint8 [B][T],
        one information bit per entry (viterbi_decode, unpacked), and, with ref_bits [B][T], nbiterr uint32 [B].
        dd_iterations n > 0 (needs rx [B][15][53], the received frames): n decision-directed rounds follow on the
        device with no host read in between -- the decoded bits are re-encoded and the channel is estimated from
        all 48 x 15 data symbols (reencode), rx is demodulated again with that estimate (no blend, tracked),
        demapped and decoded.  The first round removes the block phases a tracked demodulate gives for h and h_lt,
        the later ones those of the round before.  The pilots are tx_pilots' ([B][15][53], only the entries 5, 19,
        33 and 47 of each block are read) or 802.11's.  The dict gains "h_dd" [B][53] and "decode_dd", the last
        round's bits (and nbiterr); what it held without the rounds is unchanged."""
        eq, h = _as_c128(eq), _as_c128(h)
        B = eq.shape[0]
        if eq.shape != (B, NBLK, NSC):
            raise ValueError("eq must be [B][15][53] complex")
        if h.shape != (B, NSC) or (h_lt is not None and np.shape(h_lt) != (B, NSC)):
            raise ValueError("h / h_lt must be [B][53] complex")
        deq, dh = DeviceArray.from_numpy(eq), DeviceArray.from_numpy(h)
        dhlt = DeviceArray.from_numpy(_as_c128(h_lt)) if h_lt is not None else None
        d = self._decode_device(deq, dh, dhlt, B, modulation, rate, scale, terminated, ref_bits)
        dd = None
        if dd_iterations:
            if rx is None or np.shape(rx) != (B, NBLK, NSC):
                raise ValueError("dd_iterations needs rx [B][15][53] complex")
            if tx_pilots is not None and np.shape(tx_pilots) != (B, NBLK, NSC):
                raise ValueError("tx_pilots must be [B][15][53] complex")
            drx = DeviceArray.from_numpy(_as_c128(rx))
            if tx_pilots is not None:
                dtx = DeviceArray.from_numpy(_as_c128(tx_pilots))
            else:   # 802.11's pilots, from the re-encoder itself
                dtx = DeviceArray((B, NBLK, NSC), zero=True)
                self.reencode(d["bits"], B, modulation, rate, scale, tx=dtx)
            fr = self.frames(dtx, drx, B)
            dtheta = DeviceArray((B, NBLK), np.float64, zero=True)
            self.demodulate(fr, dh, dhlt, NSC, modulation, scale, True, True, theta=dtheta)
            dd = self._dd_device(fr, B, d["bits"], dtheta, modulation, rate, scale, terminated, d["_ref"],
                                 int(dd_iterations))
        synchronize()
        res = self._decode_result(d, modulation, rate)
        if dd is not None:
            res["h_dd"], res["decode_dd"] = self._dd_result(dd, modulation, rate)
        return res

    def mmse_solve(self, frames: Frames, W, w_stride=NSC, stream=None):
        _check(_lib.wce_mmse_solve(self.handle, byref(frames), _addr(W), w_stride, stream), "wce_mmse_solve")

    def mmse_apply(self, W, H, n_frames, stride=NSC, stream=None):
        _check(_lib.wce_mmse_apply(self.handle, _addr(W), _addr(H), stride, n_frames, stream), "wce_mmse_apply")

    def synth(self, tx, rx, rx_pre, n_frames, first_frame=0, seed=0x80211, h_shared=None, amplitude=8.8753,
              ow2=9.6172e-08, frame_stride=NBLK * NSC, block_stride=NSC, pre_stride=NSC, stream=None):
        _check(_lib.wce_synth_frames(self.handle, _addr(tx), _addr(rx), _addr(rx_pre), frame_stride, block_stride,
                                     pre_stride, first_frame, n_frames, seed, _addr(h_shared), amplitude, ow2,
                                     stream), "wce_synth_frames")

    def front_end_sync(self, capture, n_frames, capture_len, ltf, threshold, backoff=0, start=None, metric=None,
                       capture_stride=None, stream=None):
        """wce_front_end_sync: packet detection and symbol timing on raw capture windows (device)
        [n_frames][capture_stride], against ltf, one clean 64-sample period of the long training symbol
        (device).  start (device int32 [n_frames]) receives each window's packet start less backoff, or -1
        below threshold; metric (device float64 [n_frames], optional) the timing metric in [0, 1]."""
        cs = capture_stride if capture_stride is not None else capture_len
        _check(_lib.wce_front_end_sync(self.handle, _addr(capture), cs, capture_len, n_frames, _addr(ltf),
                                       threshold, backoff, _addr(start), _addr(metric), stream),
               "wce_front_end_sync")

    def front_end_sync_stf(self, capture, n_frames, capture_len, ltf, threshold_stf, threshold_ltf, backoff=0,
                           start=None, cfo=None, metric_stf=None, metric_ltf=None, capture_stride=None, stream=None):
        """wce_front_end_sync_stf: detection on the short training field at any carrier offset, the coarse offset
        from its lag-16 autocorrelation, front_end_sync's timing against ltf turned by it, and the two-copy fine
        offset unwrapped by the coarse one, on raw capture windows (device) [n_frames][capture_stride].  start
        (device int32 [n_frames]) as front_end_sync's; cfo (device float64 [n_frames]) the total offset in
        cycles per sample, |e| < 1/32, NaN where start is -1 -- to be read by front_end_preamble(start=, cfo=,
        estimate_cfo=False) and front_end_blocks(start=, cfo=).  metric_stf, metric_ltf (device float64
        [n_frames], optional): the two metrics in [0, 1]."""
        cs = capture_stride if capture_stride is not None else capture_len
        _check(_lib.wce_front_end_sync_stf(self.handle, _addr(capture), cs, capture_len, n_frames, _addr(ltf),
                                           threshold_stf, threshold_ltf, backoff, _addr(start), _addr(cfo),
                                           _addr(metric_stf), _addr(metric_ltf), stream), "wce_front_end_sync_stf")

    def front_end_blocks(self, samples, n_frames, n_blocks=NBLK, sym=None, packet_stride=None,
                         frame_stride=NBLK * NSC, block_stride=NSC, stream=None, cfo=None, sample_offset=0,
                         start=None, capture_len=None):
        """Time-domain packets (device) -> 53-bin OFDM symbols (WiFi_blocks_extraction.m).  cfo (a device
        array of n_frames doubles, cycles per sample, e.g. front_end_preamble's): wce_front_end_blocks_cfo,
        packet sample m derotated as sample m + sample_offset after the end of the long training field.
        start (device int32 [n_frames], e.g. front_end_sync's) with capture_len: wce_front_end_blocks_at,
        samples are capture windows and frame f's packet begins start[f] + 128 + sample_offset into its own."""
        if start is not None:
            if capture_len is None:
                raise ValueError("start needs capture_len")
            ps = packet_stride if packet_stride is not None else capture_len
            _check(_lib.wce_front_end_blocks_at(self.handle, _addr(samples), ps, capture_len, n_frames, n_blocks,
                                                _addr(start), _addr(cfo), sample_offset, _addr(sym), frame_stride,
                                                block_stride, stream), "wce_front_end_blocks_at")
            return
        ps = packet_stride if packet_stride is not None else SAMPLES_PER_BLOCK * n_blocks
        if cfo is None:
            _check(_lib.wce_front_end_blocks(self.handle, _addr(samples), ps, n_frames, n_blocks, _addr(sym),
                                             frame_stride, block_stride, stream), "wce_front_end_blocks")
            return
        _check(_lib.wce_front_end_blocks_cfo(self.handle, _addr(samples), ps, n_frames, n_blocks, _addr(cfo),
                                             sample_offset, _addr(sym), frame_stride, block_stride, stream),
               "wce_front_end_blocks_cfo")

    def front_end_preamble(self, lptot, n_frames, lptot_len, pre_fft, ow2=None, lptot_stride=None,
                           pre_stride=NSC, stream=None, cfo=None, estimate_cfo=True, start=None, capture_len=None):
        """Long training fields (device) -> preamble FFT [53] and sigma^2 per frame (WiFi_RX.m:18-30).  cfo (a
        device array of n_frames doubles): wce_front_end_preamble_cfo, which writes each frame's two-copy
        estimate there (estimate_cfo) or reads it, and derotates the field before anything else.
        start (device int32 [n_frames], e.g. front_end_sync's): wce_front_end_preamble_at, lptot holds capture
        windows of capture_len samples (default lptot_len) and frame f's field is the 128 samples at start[f]."""
        if start is not None:
            win = capture_len if capture_len is not None else lptot_len
            ls = lptot_stride if lptot_stride is not None else win
            _check(_lib.wce_front_end_preamble_at(self.handle, _addr(lptot), ls, win, n_frames, _addr(start),
                                                  _addr(pre_fft), pre_stride, _addr(ow2), _addr(cfo),
                                                  1 if (estimate_cfo and cfo is not None) else 0, stream),
                   "wce_front_end_preamble_at")
            return
        ls = lptot_stride if lptot_stride is not None else lptot_len
        if cfo is None:
            _check(_lib.wce_front_end_preamble(self.handle, _addr(lptot), ls, lptot_len, n_frames, _addr(pre_fft),
                                               pre_stride, _addr(ow2), stream), "wce_front_end_preamble")
            return
        _check(_lib.wce_front_end_preamble_cfo(self.handle, _addr(lptot), ls, lptot_len, n_frames, _addr(pre_fft),
                                               pre_stride, _addr(ow2), _addr(cfo), 1 if estimate_cfo else 0, stream),
               "wce_front_end_preamble_cfo")

    def front_end_host(self, packets, lptot=None, n_blocks=NBLK, cfo=False, sample_offset=0):
        """Convenience: host packets [B][80 n_blocks] (+ lptot [B][L]) -> (sym [B][n_blocks][53],
        pre_fft [B][53] or None, ow2 [B] or None).  cfo: each packet's carrier frequency offset is estimated
        from its lptot and removed from both (the packet starts sample_offset samples after the field); a
        fourth value, cfo [B] in cycles per sample, is returned."""
        packets = _as_c128(packets)
        B = packets.shape[0]
        if cfo and lptot is None:
            raise ValueError("cfo needs lptot")
        dp = DeviceArray.from_numpy(packets)
        dsym = DeviceArray((B, n_blocks, NSC), zero=True)
        dcfo = DeviceArray((B,), np.float64, zero=True) if cfo else None
        pre = ow2 = None
        if lptot is not None:
            lptot = _as_c128(lptot)
            dl = DeviceArray.from_numpy(lptot)
            dpre = DeviceArray((B, NSC), zero=True)
            dow2 = DeviceArray((B,), np.float64, zero=True)
            self.front_end_preamble(dl, B, lptot.shape[1], dpre, dow2, cfo=dcfo)
        # after the preamble on the same (null) stream: its estimate is the blocks' cfo
        self.front_end_blocks(dp, B, n_blocks, dsym, packet_stride=packets.shape[1], frame_stride=n_blocks * NSC,
                              cfo=dcfo, sample_offset=sample_offset)
        synchronize()
        sym = dsym.numpy()
        if lptot is not None:
            pre, ow2 = dpre.numpy(), dow2.numpy()
        return (sym, pre, ow2, dcfo.numpy()) if cfo else (sym, pre, ow2)

    def estimate_host(self, tx, rx, rx_pre=None, mask=ALL, block=0, eq_source=PS_LINEAR, semantics=SEM_C,
                      tx_pre=None, ls_f32=False, ow2=None):
        """Convenience: host numpy frames [B][15][53] -> dict of host outputs.  ow2: host array [B], each
        frame's own noise variance for PS_MMSE (wce_estimate_noise)."""
        tx, rx = _as_c128(tx), _as_c128(rx)
        B = tx.shape[0]
        if tx.shape != (B, NBLK, NSC) or rx.shape != tx.shape:
            raise ValueError("tx/rx must be [B][15][53] complex")
        dtx, drx = DeviceArray.from_numpy(tx), DeviceArray.from_numpy(rx)
        dpre = DeviceArray.from_numpy(_as_c128(rx_pre)) if rx_pre is not None else None
        dow2 = None
        if ow2 is not None:
            ow2 = np.ascontiguousarray(np.asarray(ow2, dtype=np.float64))
            if ow2.shape != (B,):
                raise ValueError("ow2 must be [B] float")
            dow2 = DeviceArray.from_numpy(ow2)
        dtp = DeviceArray.from_numpy(_as_c128(tx_pre)) if tx_pre is not None else None
        return self._estimate_device(dtx, drx, dpre, B, mask, block, eq_source, semantics, dtp, ls_f32, dow2)

    def _estimate_device(self, dtx, drx, dpre, B, mask, block, eq_source, semantics, dtp, ls_f32, dow2, demod=None,
                         decode=None, dd_iterations=0, tracker=None):
        """estimate_host's device half: dense [B][15][53] frames (and rx_pre [B][53], tx_pre [53], ow2 [B] or
        None) on the device -> dict of host outputs.  demod: (source bit, modulation, scale, track) queues
        demodulate behind the estimate with h = that estimator's output and h_lt = lt_ls; the dict gains "demod".
        decode (needs demod): (rate, ref_bits, terminated) queues soft_demap and viterbi_decode behind that, on
        the demodulated eq where it lies on the device; the dict gains "decode".  dd_iterations n > 0 (needs
        decode): n decision-directed rounds (_dd_device) behind that, on the decoder's bits and the demodulator's
        block phases; the dict gains "h_dd" and "decode_dd".  tracker (needs demod): (mu, beta): track_demodulate takes
        demodulate's place with h = the source's output and no h_lt, and soft_demap_blocks soft_demap's; "demod"
        gains h_blocks and h_last."""
        lsdt = np.complex64 if ls_f32 else np.complex128
        outs = {n: DeviceArray((B, NSC), np.complex128 if n == "ps_mmse" else lsdt, zero=True)
                for n, bit in _ESTIMATORS if mask & bit}
        deq = DeviceArray((B, NBLK, NSC), lsdt, zero=True) if mask & EQUALIZE else None
        o = Outputs(*[(outs[n].addr if n in outs else None) for n, _ in _ESTIMATORS],
                    deq.addr if deq is not None else None, NSC, NBLK * NSC, NSC, eq_source,
                    OUT_LS_F32 if ls_f32 else 0)
        fr = self.frames(dtx, drx, B, rx_pre=dpre, block=block, semantics=semantics, tx_pre=dtp)
        self.estimate(fr, o, mask, ow2=dow2)
        dem = dec = dd = None
        if demod is not None:   # same (null) stream: it reads the estimate's outputs in order, no host hop
            src = {bit: n for n, bit in _ESTIMATORS}[demod[0]]
            if tracker is not None:
                dem = self._track_device(fr, B, outs[src], tracker[0], tracker[1], demod[1], demod[2], demod[3], True)
            else:
                dem = self._demod_device(fr, B, outs[src], outs["lt_ls"], demod[1], demod[2], demod[3], True)
            if decode is not None:
                dec = self._decode_device(dem["eq"], outs[src], outs["lt_ls"], B, demod[1], decode[0], demod[2],
                                          decode[2], decode[1], h_blocks=dem.get("h_blocks"))
                if dd_iterations:
                    dd = self._dd_device(fr, B, dec["bits"], dem["theta"], demod[1], decode[0], demod[2], decode[2],
                                         dec["_ref"], int(dd_iterations))
        synchronize()
        res = {n: outs[n].numpy() for n in outs}
        if deq is not None:
            res["eq"] = deq.numpy()
        if dem is not None:
            res["demod"] = {n: a.numpy() for n, a in dem.items()}
        if dec is not None:
            res["decode"] = self._decode_result(dec, demod[1], decode[0])
        if dd is not None:
            res["h_dd"], res["decode_dd"] = self._dd_result(dd, demod[1], decode[0])
        return res

    @staticmethod
    def _demod_request(demod_source, mask, modulation, scale, track):
        """receive_host's demod_source: None, or one estimator bit that `mask` holds beside LT_LS"""
        if demod_source is None:
            return None
        if demod_source not in (LT_LS, PS_LINEAR, PS_CUBIC, PS_SINC, PS_MMSE):
            raise ValueError("demod_source must be one estimator bit")
        if not (mask & demod_source) or not (mask & LT_LS):
            raise ValueError("demod_source and LT_LS must be in mask")
        return (demod_source, modulation, scale, track)

    @staticmethod
    def _decode_request(decode_rate, dem, ref_bits, terminated):
        """receive_host's decode_rate: None, or a RATE_* value beside a demod_source"""
        if decode_rate is None:
            return None
        if dem is None:
            raise ValueError("decode_rate needs demod_source")
        info_bits(dem[1], decode_rate)   # raises for an unknown modulation or rate
        return (decode_rate, ref_bits, terminated)

    def receive_host(self, tx_packets, tx_lptot, rx_packets, rx_lptot, mask=ALL, semantics=SEM_MATLAB, cfo=False,
                     sample_offset=0, demod_source=None, modulation=MOD_BPSK, scale=8.8753, track=True,
                     tracker=None, decode_rate=None, ref_bits=None, terminated=True):
        """WiFi_RX.m:17-60 for a batch, on the device with no host hop in between: host time-domain packets
        [B][>= 1200] and long training fields [B][L] of both sides -> the front end (symbols, preamble FFTs and
        each packet's sigma^2) -> estimate with each frame's own rx preamble (WCE_MMSE_FRAME_COV) and own
        noise variance (wce_estimate_noise) -> dict of host outputs, plus "ow2" [B].  `mask` must hold PS_MMSE.
        Needs a WCE_MMSE_TEXTBOOK context built from the shared tx preamble: every packet carries the same
        tx long training field, and packet 0's FFT is the tx_pre of the call.
        cfo: each received packet's carrier frequency offset is estimated from its long training field and
        removed from the field and the packet (which starts sample_offset samples after the field) before
        anything else, on the same stream; the dict gains "cfo" [B], cycles per sample.  The tx side is the
        clean reference and is never derotated.
        demod_source: an estimator bit of `mask` (PS_MMSE included; LT_LS must be in mask too): the frames are
        demodulated with h = that estimator's output and h_lt = the frame's lt_ls (demodulate: `modulation`,
        `scale`, `track`, EVM against tx), queued behind the estimate; the dict gains "demod", the dict of
        demodulate_host.  None: no demodulation.
        decode_rate: a RATE_* value (demod_source must be set): the demodulated eq stays on the device and is
        demapped and decoded there (soft_demap with the same h and h_lt, viterbi_decode at that rate, `terminated`),
        queued behind the demodulation; the dict gains "decode", the dict of decode_host (nbiterr with ref_bits
        [B][T]).  A frame of NaN symbols decodes from all-zero soft bits to all-zero bits.
        tracker: (mu, beta) (demod_source must be set): the channel is tracked through the packet --
        track_demodulate takes demodulate's place, starting from h = that estimator's output with no h_lt blend
        (`track` is its phase flag), and with a decode_rate soft_demap_blocks takes soft_demap's with the estimate
        of each block; "demod" gains h_blocks and h_last.  None: the calls and bits above."""
        if tracker is not None:
            if demod_source is None or len(tracker) != 2:
                raise ValueError("tracker is (mu, beta) and needs demod_source")
            tracker = (float(tracker[0]), int(tracker[1]))
        return self._receive_host(tx_packets, tx_lptot, rx_packets, rx_lptot, mask, semantics, cfo, sample_offset,
                                  demod_source, modulation, scale, track, decode_rate, ref_bits, terminated, 0,
                                  tracker)

    def receive_iterated_host(self, tx_packets, tx_lptot, rx_packets, rx_lptot, demod_source, decode_rate,
                              dd_iterations=1, **receive):
        """receive_host(tx_packets, tx_lptot, rx_packets, rx_lptot, demod_source=..., decode_rate=..., **receive)
        with dd_iterations decision-directed rounds queued behind its decoder, on the same stream with no host
        read in between: the decoded bits are re-encoded and the channel is estimated from all 48 x 15 data
        symbols, with the block phases the demodulator tracked removed (reencode; the pilots are the tx side's),
        the frames are demodulated again with that estimate (no blend, tracked), demapped and decoded, each round
        on the bits and phases of the one before.  -> receive_host's dict, unchanged, plus "h_dd" [B][53] and
        "decode_dd", the last round's bits (and nbiterr with ref_bits).  dd_iterations 0: receive_host's dict."""
        names = ("mask", "semantics", "cfo", "sample_offset", "modulation", "scale", "track", "ref_bits", "terminated")
        unknown = set(receive) - set(names)
        if unknown:
            raise TypeError(f"receive_iterated_host: unknown keywords {sorted(unknown)}")
        if dd_iterations < 0 or decode_rate is None:
            raise ValueError("receive_iterated_host needs a decode_rate and dd_iterations >= 0")
        kw = dict(mask=ALL, semantics=SEM_MATLAB, cfo=False, sample_offset=0, modulation=MOD_BPSK, scale=8.8753,
                  track=True, ref_bits=None, terminated=True)
        kw.update(receive)
        return self._receive_host(tx_packets, tx_lptot, rx_packets, rx_lptot, kw["mask"], kw["semantics"], kw["cfo"],
                                  kw["sample_offset"], demod_source, kw["modulation"], kw["scale"], kw["track"],
                                  decode_rate, kw["ref_bits"], kw["terminated"], int(dd_iterations))

    def _receive_host(self, tx_packets, tx_lptot, rx_packets, rx_lptot, mask, semantics, cfo, sample_offset,
                      demod_source, modulation, scale, track, decode_rate, ref_bits, terminated, dd_iterations,
                      tracker=None):
        """receive_host's body; dd_iterations: the decision-directed rounds of receive_iterated_host"""
        dem = self._demod_request(demod_source, mask, modulation, scale, track)
        dcd = self._decode_request(decode_rate, dem, ref_bits, terminated)
        pk = [_as_c128(tx_packets), _as_c128(rx_packets)]
        lp = [_as_c128(tx_lptot), _as_c128(rx_lptot)]
        B = pk[1].shape[0]
        if any(p.ndim != 2 or p.shape[0] != B or p.shape[1] < SAMPLES_PER_BLOCK * NBLK for p in pk):
            raise ValueError("packets must be [B][>= 1200] complex")
        if any(l.ndim != 2 or l.shape[0] != B for l in lp):
            raise ValueError("lptot must be [B][L] complex")
        sym, pre, keep = [], [], []
        dow2 = DeviceArray((B,), np.float64, zero=True)
        dcfo = DeviceArray((B,), np.float64, zero=True) if cfo else None
        for side in (0, 1):
            dp, dl = DeviceArray.from_numpy(pk[side]), DeviceArray.from_numpy(lp[side])
            keep += [dp, dl]   # read by the queued front end until _estimate_device synchronises
            dsym, dpre = DeviceArray((B, NBLK, NSC), zero=True), DeviceArray((B, NSC), zero=True)
            if side == 1 and cfo:   # the preamble's estimate first: the blocks read it
                self.front_end_preamble(dl, B, lp[side].shape[1], dpre, dow2, cfo=dcfo)
                self.front_end_blocks(dp, B, NBLK, dsym, packet_stride=pk[side].shape[1], cfo=dcfo,
                                      sample_offset=sample_offset)
            else:
                self.front_end_blocks(dp, B, NBLK, dsym, packet_stride=pk[side].shape[1])
                self.front_end_preamble(dl, B, lp[side].shape[1], dpre, dow2 if side == 1 else None)
            sym.append(dsym)
            pre.append(dpre)
        # same (null) stream throughout: the estimate reads the front end's outputs in order
        res = self._estimate_device(sym[0], sym[1], pre[1], B, mask | FRAME_COV, 0, PS_LINEAR, semantics, pre[0],
                                    False, dow2, dem, dcd, dd_iterations, tracker)
        res["ow2"] = dow2.numpy()
        if cfo:
            res["cfo"] = dcfo.numpy()
        return res

    def receive_capture_host(self, tx_packets, tx_lptot, rx_capture, threshold, backoff=0, mask=ALL,
                             semantics=SEM_MATLAB, cfo=False, sample_offset=0, demod_source=None,
                             modulation=MOD_BPSK, scale=8.8753, track=True, stf=False, stf_threshold=0.25,
                             decode_rate=None, ref_bits=None, terminated=True):
        """receive_host with the rx side taken from raw capture windows [B][capture_len], in which each packet
        (long training field, then sample_offset samples, then the packet) starts at an unknown sample:
        front_end_sync against tx_lptot[0][-64:] finds each window's start (start - backoff, or -1 where the
        metric stays below threshold), the front end reads field and packet there, and the estimate follows,
        all queued on one stream with no host hop.  The dict gains "start" [B] int32 and "metric" [B]; a
        window without a detected packet, or one the packet does not fit in, gives NaN rows.
        demod_source, modulation, scale, track: as receive_host; such a window's "demod" has NaN evm and
        0xFF symbols.  decode_rate, ref_bits, terminated: as receive_host; such a window's "decode" has
        all-zero soft bits and all-zero bits.
        stf: the windows' packets carry a short training field (transmit_host(stf=True)): front_end_sync_stf
        (thresholds stf_threshold and threshold) finds start and the carrier offset, |cfo| < 1/32 cycles per
        sample, which is removed whatever `cfo` says; the dict gains "cfo" and "metric_stf", and "metric" is
        the long field's."""
        dem = self._demod_request(demod_source, mask, modulation, scale, track)
        dcd = self._decode_request(decode_rate, dem, ref_bits, terminated)
        pk, lp, cap = _as_c128(tx_packets), _as_c128(tx_lptot), _as_c128(rx_capture)
        if cap.ndim != 2 or cap.shape[1] < 2 * FFT_SIZE:
            raise ValueError("rx_capture must be [B][>= 128] complex")
        B, W = cap.shape
        if pk.ndim != 2 or pk.shape[0] != B or pk.shape[1] < SAMPLES_PER_BLOCK * NBLK:
            raise ValueError("tx_packets must be [B][>= 1200] complex")
        if lp.ndim != 2 or lp.shape[0] != B or lp.shape[1] < 2 * FFT_SIZE:
            raise ValueError("tx_lptot must be [B][>= 128] complex")
        dpk, dlp, dcap = DeviceArray.from_numpy(pk), DeviceArray.from_numpy(lp), DeviceArray.from_numpy(cap)
        dltf = DeviceArray.from_numpy(np.ascontiguousarray(lp[0, -FFT_SIZE:]))
        sym, pre = DeviceArray((B, NBLK, NSC), zero=True), DeviceArray((B, NSC), zero=True)
        self.front_end_blocks(dpk, B, NBLK, sym, packet_stride=pk.shape[1])
        self.front_end_preamble(dlp, B, lp.shape[1], pre, None)
        # same (null) stream throughout: each call reads what the one before wrote
        f = self._capture_front(dcap, B, W, dltf, threshold, backoff, stf, stf_threshold, cfo, sample_offset)
        res = self._estimate_device(sym, f["rx"], f["rx_pre"], B, mask | FRAME_COV, 0, PS_LINEAR, semantics, pre,
                                    False, f["ow2"], dem, dcd)
        for n in ("ow2", "cfo", "start", "metric", "metric_stf"):
            if f.get(n) is not None:
                res[n] = f[n].numpy()
        return res


class Plan:
    """wce_plan: a captured wce_estimate call, replayed with one graph launch.
    Keeps references to the frames/outputs structs (the buffers they point
    to must outlive the plan)."""

    def __init__(self, ctx, frames, outputs, mask):
        self.handle = c_void_p()
        self._keep = (ctx, frames, outputs)
        _check(_lib.wce_plan_create(byref(self.handle), ctx.handle, byref(frames), byref(outputs), mask),
               "wce_plan_create")

    def launch(self, stream=None):
        _check(_lib.wce_plan_launch(self.handle, stream), "wce_plan_launch")

    def close(self):
        if self.handle is not None and self.handle.value:
            _lib.wce_plan_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass


def pdp_taps(rng, n_frames, power) -> np.ndarray:
    """Channel taps for Context.transmit_host / link_host from a power-delay profile: tap t of each of n_frames
    frames is drawn CN(0, power[t]) from rng (a numpy Generator), and each frame's taps are then normalised to
    sum |h|^2 = 1 -> complex [n_frames][len(power)], 1..16 taps.  np.diag(power), zero-padded to 53 x 53 (for a
    profile that sums to 1), is the Rhh that Context(Rhh=...) takes, so a matched-model WCE_MMSE_COV run is
        R = np.zeros((53, 53), complex); R[:len(power), :len(power)] = np.diag(power)
        ctx = Context(tx_pre, rx_pre, ow2, Rhh=R)
        ctx.link_host(modulation, rate, snr_db, B, taps=pdp_taps(rng, B, power))"""
    power = np.asarray(power, np.float64)
    if power.ndim != 1 or not 1 <= power.size <= 16 or np.any(power < 0) or not power.sum() > 0:
        raise ValueError("power must hold 1..16 non-negative tap powers")
    h = (rng.standard_normal((n_frames, power.size)) + 1j * rng.standard_normal((n_frames, power.size))) * \
        np.sqrt(power / 2)
    return h / np.sqrt(np.sum(np.abs(h) ** 2, axis=1, keepdims=True))


def fading_taps(rng, n_frames, power, rho, n_knots) -> np.ndarray:
    """Tap trajectories for Context.transmit_host / link_host (3-D taps): knot 0 is pdp_taps(rng, n_frames, power),
    drawn from the same generator state in the same order and normalised the same way, and each further knot is
    the Gauss-Markov step  knot k+1 = rho knot k + sqrt(1 - rho^2) w c,  w drawn CN(0, power) per tap and c the
    factor that normalised knot 0 -- so every knot of a tap has the variance of knot 0 and neighbouring knots
    correlate by rho.  rho in [0, 1]: 1.0 freezes the channel (every knot is knot 0, bit for bit).
    -> complex [n_frames][n_knots][len(power)]; the transmitter interpolates linearly between the knots."""
    if not 0.0 <= rho <= 1.0:
        raise ValueError("rho must lie in [0, 1]")
    if n_knots < 2:
        raise ValueError("n_knots must be at least 2")
    power = np.asarray(power, np.float64)
    if power.ndim != 1 or not 1 <= power.size <= 16 or np.any(power < 0) or not power.sum() > 0:
        raise ValueError("power must hold 1..16 non-negative tap powers")
    shape = (n_frames, power.size)
    h = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(power / 2)
    c = 1.0 / np.sqrt(np.sum(np.abs(h) ** 2, axis=1, keepdims=True))
    out = np.empty((n_frames, n_knots, power.size), np.complex128)
    out[:, 0] = h / np.sqrt(np.sum(np.abs(h) ** 2, axis=1, keepdims=True))
    step = np.sqrt(1.0 - rho * rho)
    for k in range(1, n_knots):
        w = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(power / 2)
        out[:, k] = rho * out[:, k - 1] + step * w * c
    return out


def state_blob(tx_pre, rx_pre, ow2, mode=MMSE_REF, Rhh=None) -> np.ndarray:
    """The shared state built on the host (no device): bytes to broadcast."""
    lib = load()
    n = lib.wce_state_size()
    blob = np.zeros(n, np.uint8)
    tp, rp = _as_c128(tx_pre), _as_c128(rx_pre)
    if Rhh is not None:
        R = _as_c128(Rhh)
        _check(lib.wce_state_build_cov(blob.ctypes.data_as(c_void_p), n, tp.ctypes.data_as(c_void_p),
                                       rp.ctypes.data_as(c_void_p), R.ctypes.data_as(c_void_p), float(ow2)),
               "wce_state_build_cov")
        return blob
    _check(lib.wce_state_build(blob.ctypes.data_as(c_void_p), n, tp.ctypes.data_as(c_void_p),
                               rp.ctypes.data_as(c_void_p), float(ow2), mode), "wce_state_build")
    return blob


def state_mode(blob: np.ndarray) -> int:
    """The MMSE mode of a valid state blob (wce_state_validate); raises if the bytes hold no state."""
    m = c_int()
    _check(load().wce_state_validate(blob.ctypes.data_as(c_void_p), blob.nbytes, byref(m)), "wce_state_validate")
    return m.value


def debug_route(mode, bdot, fuse, cm, lr_k0, rank, sem, mask, f32, r1, ref_fc, ref_ls, noise=False) -> str:
    """The kernel families one estimate call with these facts launches, in order, ';'-separated
    (wce_debug_route: the route planner alone, no device); raises WceError for facts validation rejects.
    noise: the call carries per-frame ow2 (wce_estimate_noise; wce_debug_route_noise plans it)."""
    buf = ctypes.create_string_buffer(256)
    facts = (int(mode), int(bdot), int(fuse), int(cm), int(lr_k0), int(rank), int(sem), int(mask), int(f32), int(r1),
             int(ref_fc), int(ref_ls))
    if noise:
        _check(load().wce_debug_route_noise(*facts, 1, buf, len(buf)), "wce_debug_route_noise")
    else:
        _check(load().wce_debug_route(*facts, buf, len(buf)), "wce_debug_route")
    return buf.value.decode()


def cov_factor(blob: np.ndarray):
    """A WCE_MMSE_COV state blob's low-rank factor: (U [53 x rank] with C = U U^H, rank, k0, lambda_max,
    lambda_min); k0 = -1 when the dense Ryy solve runs, else the Gram system's first block row."""
    U = np.zeros((NSC, 64), np.complex128)
    r, k0 = c_int(), c_int()
    lmax, lmin = c_double(), c_double()
    _check(load().wce_debug_cov_factor(blob.ctypes.data_as(c_void_p), blob.nbytes, U.ctypes.data_as(c_void_p),
                                       byref(r), byref(k0), byref(lmax), byref(lmin)), "wce_debug_cov_factor")
    return U[:, :r.value].copy(), r.value, k0.value, lmax.value, lmin.value


def ldc_to_complex(src, dst, n, stream=None):
    """wce_ldc_to_complex: n long double _Complex values (the reference's
    format, raw x87 bytes in device memory, e.g. DeviceArray of clongdouble)
    -> complex double in dst, rounded as C's (double) cast."""
    _check(load().wce_ldc_to_complex(_addr(src), _addr(dst), int(n), stream), "wce_ldc_to_complex")


def complex_to_ldc(src, dst, n, stream=None):
    """wce_complex_to_ldc: n complex double -> long double _Complex (exact)."""
    _check(load().wce_complex_to_ldc(_addr(src), _addr(dst), int(n), stream), "wce_complex_to_ldc")


def synchronize(stream=None):
    _check(load().wce_stream_synchronize(stream), "wce_stream_synchronize")


class Stream:
    def __init__(self):
        self.handle = c_void_p()
        _check(load().wce_stream_create(byref(self.handle)), "wce_stream_create")

    def synchronize(self):
        _check(_lib.wce_stream_synchronize(self.handle), "wce_stream_synchronize")

    def __del__(self):
        try:
            if self.handle.value:
                _lib.wce_stream_destroy(self.handle)
        except Exception:  # pragma: no cover
            pass


class Event:
    def __init__(self):
        self.handle = c_void_p()
        _check(load().wce_event_create(byref(self.handle)), "wce_event_create")

    def record(self, stream=None):
        s = stream.handle if isinstance(stream, Stream) else stream
        _check(_lib.wce_event_record(self.handle, s), "wce_event_record")

    def query(self) -> bool:
        """wce_event_query: True once the work in front of the recorded event has completed; never waits."""
        rc = _lib.wce_event_query(self.handle)
        if rc < 0:
            raise WceError(rc, "wce_event_query")
        return rc == 1

    def elapsed_ms(self, end: "Event") -> float:
        ms = ctypes.c_float()
        _check(_lib.wce_event_elapsed_ms(byref(ms), self.handle, end.handle), "wce_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            if self.handle.value:
                _lib.wce_event_destroy(self.handle)
        except Exception:  # pragma: no cover
            pass


# ------------------------------------------------------------------------
# The reference's entry points (main.c:4-8): same names, same argument
# meaning, results written into H_EST (53 complex).  Arrays are numpy
# clongdouble (= long double _Complex) or anything convertible.
# ------------------------------------------------------------------------
def _ld(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.clongdouble))


def _call_compat(name, *arrays, out):
    lib = load()
    ins = [_ld(a) for a in arrays]
    if any(a.shape[0] < NSC for a in ins):
        raise ValueError("estimator inputs need 53 subcarriers")
    res = np.zeros(NSC, np.clongdouble)
    getattr(lib, name)(*[a.ctypes.data_as(c_void_p) for a in ins], res.ctypes.data_as(c_void_p))
    _check(lib.wce_compat_last_status(), name)
    if out is not None:
        out[:NSC] = res
    return res


def WiFi_channel_estimation_LT_LS(tx_pre, rx_pre, H_EST=None):
    """main.c:66-75 on the GPU."""
    return _call_compat("WiFi_channel_estimation_LT_LS", tx_pre, rx_pre, out=H_EST)


def WiFi_channel_estimation_PS_Linear(tx_symbols, rx_symbols, H_EST=None):
    """main.c:77-101 on the GPU."""
    return _call_compat("WiFi_channel_estimation_PS_Linear", tx_symbols, rx_symbols, out=H_EST)


def WiFi_channel_estimation_PS_Cubic(tx_symbols, rx_symbols, H_EST=None):
    """main.c:103-122 on the GPU."""
    return _call_compat("WiFi_channel_estimation_PS_Cubic", tx_symbols, rx_symbols, out=H_EST)


def WiFi_channel_estimation_PS_Sinc(tx_symbols, rx_symbols, H_EST=None):
    """main.c:124-146 on the GPU."""
    return _call_compat("WiFi_channel_estimation_PS_Sinc", tx_symbols, rx_symbols, out=H_EST)


def WiFi_channel_estimation_PS_MMSE(tx_symbols, rx_symbols, F, ow2, H_EST_LS, H_EST=None):
    """main.c:148-212 (REF-repaired) on the GPU.  F: 53x53."""
    lib = load()
    tx, rx, hls = _ld(tx_symbols), _ld(rx_symbols), _ld(H_EST_LS)
    Fm = np.ascontiguousarray(np.asarray(F, dtype=np.clongdouble).reshape(NSC, NSC))
    rows = (c_void_p * NSC)(*[Fm[i].ctypes.data for i in range(NSC)])
    res = np.zeros(NSC, np.clongdouble)
    lib.WiFi_channel_estimation_PS_MMSE(tx.ctypes.data_as(c_void_p), rx.ctypes.data_as(c_void_p),
                                        ctypes.cast(rows, c_void_p), float(ow2), hls.ctypes.data_as(c_void_p),
                                        res.ctypes.data_as(c_void_p))
    _check(lib.wce_compat_last_status(), "WiFi_channel_estimation_PS_MMSE")
    if H_EST is not None:
        H_EST[:NSC] = res
    return res
