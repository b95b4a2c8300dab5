"""ctypes binding of libravvent_hip.so (include/ravvent_hip.h).  Fails loudly: there is no
CPU fallback anywhere behind this module."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_void_p

from .config import CRvConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libravvent_hip.so")

RV_OK = 0
ERROR_NAMES = {-1: "RV_EINVAL", -2: "RV_ENOMEM", -3: "RV_EHIP", -4: "RV_ESTATE", -5: "RV_EUNSUPPORTED"}



class CRvBeams(ctypes.Structure):
    """RvBeams (include/ravvent_hip.h): the five outputs of the rv_beam_search_all* calls; the last three may be None."""
    _fields_ = [("tokens", c_void_p), ("scores", c_void_p), ("path_scores", c_void_p), ("log_probs", c_void_p), ("lengths", c_void_p)]


class CRvMoves(ctypes.Structure):
    """RvMoves (include/ravvent_hip.h): the six outputs [B, L-1, W] of the rv_beam_search_moves* calls; each may be None, not all."""
    _fields_ = [("raw_pos", c_void_p), ("raw_mass", c_void_p), ("event_pos", c_void_p), ("event_mass", c_void_p), ("peak", c_void_p),
                ("peak_weight", c_void_p)]


class CRvCallMoves(ctypes.Structure):
    """RvCallMoves (include/ravvent_hip.h): the six outputs [B, L-1] of the rv_beam_search_*calls_moves calls; each may be None, not all."""
    _fields_ = CRvMoves._fields_


class CRvScore(ctypes.Structure):
    """RvScore (include/ravvent_hip.h): the outputs of rv_teacher_forced* / rv_score_logits; each may be None."""
    _fields_ = [("nll", c_void_p), ("nll_sum", c_void_p), ("n_labels", c_void_p), ("n_match", c_void_p), ("n_counted", c_void_p)]


class CRvSignalPrep(ctypes.Structure):
    """RvSignalPrep (include/ravvent_hip.h): the detector's and the chunker's parameters of rv_read_put_signals."""
    _fields_ = [("window_length1", c_int32), ("window_length2", c_int32), ("threshold1", c_double), ("threshold2", c_double),
                ("peak_height", c_double), ("stride", c_int32), ("max_raw_len", c_int32), ("max_event_len", c_int32)]


class CRvStitchIn(ctypes.Structure):
    """RvStitchIn (include/ravvent_hip.h): the call tables [n, stride] / [n] and the window table [n,5] of rv_stitch_calls."""
    _fields_ = [("bases", c_void_p), ("probs", c_void_p), ("lengths", c_void_p), ("raw_pos", c_void_p), ("raw_mass", c_void_p),
                ("event_pos", c_void_p), ("event_mass", c_void_p), ("win", c_void_p), ("n", c_int32), ("stride", c_int32)]


class CRvStitchOut(ctypes.Structure):
    """RvStitchOut (include/ravvent_hip.h): the seven per-base outputs of a stitch (each may be None), their capacity in elements, and
    read_offsets i64 [n_reads + 1]."""
    _fields_ = [("bases", c_void_p), ("probs", c_void_p), ("positions", c_void_p), ("raw_mass", c_void_p), ("event_mass", c_void_p),
                ("source_chunk", c_void_p), ("source_index", c_void_p), ("capacity", c_size_t), ("read_offsets", c_void_p)]


# rv_read_fetch: which table
RV_FETCH_WINDOWS, RV_FETCH_RAW_SC, RV_FETCH_EVENTS_SC, RV_FETCH_EVENT_START, RV_FETCH_EVENT_LENGTH, RV_FETCH_EVENT_MEAN, \
    RV_FETCH_EVENT_STDV = range(7)


# every symbol include/ravvent_hip.h declares: (name, restype, argtypes)
_F, _I = POINTER(c_float), POINTER(c_int32)
_B = POINTER(CRvBeams)
_S = POINTER(CRvScore)
_M = POINTER(CRvMoves)
_CM = POINTER(CRvCallMoves)
SYMBOLS = [
    ("rv_abi_version", c_int32, []),
    ("rv_create", c_int32, [POINTER(CRvConfig), POINTER(c_void_p)]),
    ("rv_create_rnn", c_int32, [POINTER(CRvConfig), c_int32, POINTER(c_void_p)]),
    ("rv_destroy", None, [c_void_p]),
    ("rv_last_error", c_char_p, [c_void_p]),
    ("rv_weight_count", c_size_t, [c_void_p]),
    ("rv_load_weights", c_int32, [c_void_p, c_void_p, c_size_t]),
    ("rv_beam_search", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, _I]),
    ("rv_beam_search_dev", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, _I]),
    ("rv_beam_search_calls", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, _I]),
    ("rv_beam_search_submit", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, _I]),
    ("rv_beam_search_collect", c_int32, [c_void_p, c_int32, c_void_p, c_void_p, _I]),
    ("rv_beam_search_submit_dev", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, _I]),
    ("rv_beam_search_collect_dev", c_int32, [c_void_p, c_int32, _I]),
    ("rv_beam_search_submit_calls", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, _I]),
    ("rv_beam_search_collect_calls", c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, _I]),
    ("rv_beam_search_all", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, _B, _I]),
    ("rv_beam_search_all_dev", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, _B, _I]),
    ("rv_beam_search_submit_all", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, _I]),
    ("rv_beam_search_collect_all", c_int32, [c_void_p, c_int32, _B, _I]),
    ("rv_beam_search_submit_all_dev", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, _B, _I]),
    ("rv_beam_search_moves", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, _B, _M, _I]),
    ("rv_beam_search_moves_dev", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, _B, _M, _I]),
    ("rv_beam_search_submit_moves", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, _I]),
    ("rv_beam_search_collect_moves", c_int32, [c_void_p, c_int32, _B, _M, _I]),
    ("rv_beam_search_calls_moves", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, _CM, _I]),
    ("rv_beam_search_windows_calls_moves", c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, _CM, _I]),
    ("rv_beam_search_submit_windows_calls_moves", c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, _I]),
    ("rv_beam_search_collect_calls_moves", c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, _CM, _I]),
    ("rv_beam_search_flush", c_int32, [c_void_p]),
    ("rv_read_put", c_int32, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, _I]),
    ("rv_read_put_dev", c_int32, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, _I]),
    ("rv_read_drop", c_int32, [c_void_p, c_int32]),
    ("rv_read_put_signals", c_int32, [c_void_p, c_int32, c_void_p, c_void_p, POINTER(CRvSignalPrep), c_void_p, c_void_p, c_void_p]),
    ("rv_read_fetch", c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_size_t]),
    ("rv_beam_search_windows", c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, _I]),
    ("rv_beam_search_windows_dev", c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, _I]),
    ("rv_beam_search_windows_calls", c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, _I]),
    ("rv_beam_search_submit_windows", c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, _I]),
    ("rv_beam_search_submit_windows_calls", c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, _I]),
    ("rv_read_put_events", c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_size_t]),
    ("rv_stitch_calls", c_int32, [c_void_p, POINTER(CRvStitchIn), c_int32, c_void_p, POINTER(CRvStitchOut)]),
    ("rv_stitch_open", c_int32, [c_void_p, c_int32, c_int32, POINTER(c_void_p)]),
    ("rv_stitch_close", c_int32, [c_void_p, c_void_p]),
    ("rv_beam_search_submit_windows_stitch", c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                                       c_int32, _I]),
    ("rv_beam_search_collect_stitch", c_int32, [c_void_p, c_int32, _I]),
    ("rv_stitch_run", c_int32, [c_void_p, c_void_p, c_int32, c_void_p, POINTER(CRvStitchOut)]),
    ("rv_greedy_search", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, _I]),
    ("rv_greedy_search_dev", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, _I]),
    ("rv_teacher_forced", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, ctypes.c_uint32, c_void_p, c_void_p, _S]),
    ("rv_teacher_forced_dev", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, ctypes.c_uint32, c_void_p, c_void_p, _S]),
    ("rv_teacher_forced_moves", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, ctypes.c_uint32, c_void_p, c_void_p, _S, _M]),
    ("rv_teacher_forced_moves_dev", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, ctypes.c_uint32, c_void_p, c_void_p, _S, _M]),
    ("rv_score_logits", c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, ctypes.c_uint32, c_void_p, _S]),
    ("rv_set_option", c_int32, [c_void_p, c_char_p, c_int32]),
    ("rv_get_tensor", c_int32, [c_void_p, c_char_p, c_void_p, c_size_t, POINTER(c_size_t)]),
    ("rv_get_profile", c_int32, [c_void_p, c_char_p, POINTER(c_double), POINTER(c_int64)]),
    ("rv_profile_names", c_int32, [c_void_p, ctypes.c_char_p, c_size_t]),
    ("rv_reset_profile", c_int32, [c_void_p]),
    ("rv_detect_events", c_int32, [c_void_p, c_size_t, c_int32, c_int32, c_double, c_double, c_double,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, POINTER(c_size_t)]),
    ("rv_round_weights", c_int32, [c_void_p, c_void_p, c_void_p, c_size_t]),
    # include/ravvent_merge.h
    ("rv_merge_calls", c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                 c_int64, POINTER(c_int64)]),
    ("rv_merger_create", c_int32, [c_int32, c_int32, POINTER(c_void_p)]),
    ("rv_merger_append", c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32]),
    ("rv_merger_result", c_int32, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(c_int64)]),
    ("rv_merger_destroy", None, [c_void_p]),
    ("rv_merger_sources", c_int32, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(c_int64)]),
    ("rv_local_align", c_int32, [c_char_p, c_int32, c_char_p, c_int32, c_int32, c_char_p, c_char_p, c_int32, _I,
                                 POINTER(c_double), _I, _I]),
]

_lib = None


class RavventHipError(RuntimeError):
    pass


def load_library(path: str | None = None):
    """Load libravvent_hip.so and bind every declared symbol.  Raises if the library has not
    been built (run ``python -c 'import __graft_entry__ as g; g.build()'`` or ``make -C
    ravvent-basecaller_amd/csrc``)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("RAVVENT_HIP_LIB") or LIB_PATH     # RAVVENT_HIP_LIB: an alternative build of the same ABI (A/B timing)
    if not os.path.exists(p):
        raise RavventHipError(f"{p} not found: build the HIP library first (there is no CPU fallback)")
    try:   # torch bundles its own libamdhip64.so.7; load it first so both share one HIP runtime
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover
        pass
    lib = ctypes.CDLL(p)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)       # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def check(lib, handle, rc: int, what: str):
    if rc != RV_OK:
        msg = lib.rv_last_error(handle)
        raise RavventHipError(f"{what}: {ERROR_NAMES.get(rc, rc)}: {msg.decode() if msg else ''}")
