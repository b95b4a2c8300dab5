"""`Basecaller`: the reference's class API (/root/reference/basecaller.py:156-416) in front of
the HIP path.  Same constructor signature, same method names, argument meaning and return
shapes as the two evaluators rely on (ravvent_performance_evaluator.py:91-107,51-67;
SURVEY.md 8b); every number is produced by libravvent_hip.so on the GPU.

Returned tensors are ``torch.Tensor`` (they support ``.numpy()`` like the TF tensors the
callers expect).  Inputs may be numpy arrays or torch tensors, host or device; host inputs go
through the host-buffer C entry points (PCIe copies included), CUDA/HIP tensors through the
``*_dev`` entry points with no host round trip.
"""
from __future__ import annotations

import collections
import ctypes
import os

import numpy as np
import torch

from . import _capi, data_loader as _dl, weights as _weights
from .config import RvConfig, RAW_FEATURES, EVENT_FEATURES, RNNS
from .data_loader import _ASCII, nuc_tk, tokens_to_strings


# What TFA's BeamSearchDecoder returns for a slab (rv_beam_search_all*, include/ravvent_hip.h): tokens [B,S,W] int32 the W
# back-traced hypotheses, scores [B,S,W] the per-slot cumulative log-probabilities (not back-traced), path_scores [B,S,W] each
# hypothesis's own cumulative log-probability, log_probs [B,W] / lengths [B,W] the final state's
BeamHypotheses = collections.namedtuple("BeamHypotheses", "tokens scores path_scores log_probs lengths")

# Where in the chunk's signal the tokens of BeamHypotheses.tokens come from (rv_beam_search_moves*, include/ravvent_hip.h: RvMoves):
# six [B,S,W] tensors, column t of hypothesis w from the attention weights of the step that produced tokens[b, t, w]
Moves = collections.namedtuple("Moves", "raw_pos raw_mass event_pos event_mass peak peak_weight")

# What a forced decode or a scoring call leaves (rv_teacher_forced*, rv_score_logits; include/ravvent_hip.h: RvScore): sample_id [B,S]
# int32 the argmax of logits [B,S,V]; nll [B,S] f32 the masked cross-entropy terms; nll_sum [B] f32, n_labels / n_match / n_counted [B] int32
ForcedScores = collections.namedtuple("ForcedScores", "sample_id logits nll nll_sum n_labels n_match n_counted")


# The same six values per LETTER of each chunk's call (rv_beam_search_*calls_moves, include/ravvent_hip.h: RvCallMoves): numpy arrays
# [B, L-1] beside the call arrays; element i < lengths[b] belongs to letter i of chunk b, the tail holds -1 / 0
CallMoves = collections.namedtuple("CallMoves", "raw_pos raw_mass event_pos event_mass peak peak_weight")


# What a stitch by signal position returns (rv_stitch_calls / rv_stitch_run, include/ravvent_hip.h: RvStitchOut): seven arrays with one
# element per kept base -- bases u8, probs f32, positions f64, raw_mass / event_mass f32, source_chunk / source_index int32 -- and
# read_offsets int64 [n_reads + 1]: read r is elements read_offsets[r] .. read_offsets[r+1] - 1
StitchedCalls = collections.namedtuple("StitchedCalls", "bases probs positions raw_mass event_mass source_chunk source_index read_offsets")


def raw_position_estimate(raw_start, raw_pos, offset=0):
    """Position of a base in samples of the signal from the raw segment of its chunk: raw_start + raw_pos (+ the sample of the signal
    at which the scaled raw table starts); NaN stays NaN.  f64."""
    return np.asarray(raw_start, np.float64) + np.asarray(raw_pos, np.float64) + float(offset)


def event_position_estimate(event_start, event_pos, ev_starts, ev_lengths):
    """... from the event segment: e = event_start + event_pos in events of the read, i = floor(e) clipped to the read's events,
    c_j = start_j + length_j / 2 the centre of event j, estimate = c_i + (e - i) (c_min(i+1, E-1) - c_i): linear between the centres
    of neighbouring events, the last event's centre at and beyond it.  NaN stays NaN (and a read without events gives NaN).  f64."""
    e = np.asarray(event_start, np.float64) + np.asarray(event_pos, np.float64)
    c = np.asarray(ev_starts, np.float64) + np.asarray(ev_lengths, np.float64) / 2.0
    out = np.full(e.shape, np.nan, np.float64)
    E = int(c.shape[0])
    ok = ~np.isnan(e)
    if E == 0 or not ok.any():
        return out
    i = np.clip(np.floor(e[ok]), 0, E - 1).astype(np.int64)
    j = np.minimum(i + 1, E - 1)
    out[ok] = c[i] + (e[ok] - i) * (c[j] - c[i])
    return out


def signal_positions(mode, raw_start, event_start, raw_pos, raw_mass, event_pos, event_mass, ev_starts, ev_lengths, offset=0):
    """The position of each base in samples of the signal as passed in: raw mode takes the raw estimate,
    event mode the event estimate, joint mode the raw estimate where raw_mass >= event_mass and the event estimate elsewhere.
    Reported as computed: nothing forces the positions of consecutive bases to rise."""
    if mode == "raw":
        return raw_position_estimate(raw_start, raw_pos, offset)
    ev = event_position_estimate(event_start, event_pos, ev_starts, ev_lengths)
    if mode == "event":
        return ev
    take_raw = np.asarray(raw_mass, np.float32) >= np.asarray(event_mass, np.float32)
    return np.where(take_raw, raw_position_estimate(raw_start, raw_pos, offset), ev)


def phred_qualities(probs) -> np.ndarray:
    """Per-base probabilities -> Phred values u8: p clipped to [0, 1], round(-10 log10(max(1 - p, 1e-4))), clipped to [0, 40]."""
    p = np.clip(np.asarray(probs, np.float64), 0.0, 1.0)
    q = np.round(-10.0 * np.log10(np.maximum(1.0 - p, 1e-4)))
    return np.clip(q, 0, 40).astype(np.uint8)


class BasecallResult:
    """What `Basecaller.basecall` returns for a read: seq, probs (the merger's per-base probabilities, f32), qualities (their
    Phred values, u8), chunks_num.  With moves=True also, one per base of seq: positions (f64, samples of the signal as passed in;
    `signal_positions`), raw_mass / event_mass (f32, the attention weight on each segment of the base's chunk), source_chunk /
    source_index (int32: the chunk of the read the merger took the base from and its index in that chunk's call); None otherwise."""
    __slots__ = ("seq", "probs", "qualities", "chunks_num", "positions", "raw_mass", "event_mass", "source_chunk", "source_index")

    def __init__(self, seq, probs, chunks_num, positions=None, raw_mass=None, event_mass=None, source_chunk=None, source_index=None):
        self.seq = seq
        self.probs = np.asarray(probs, np.float32)
        self.qualities = phred_qualities(self.probs)
        self.chunks_num = int(chunks_num)
        self.positions, self.raw_mass, self.event_mass = positions, raw_mass, event_mass
        self.source_chunk, self.source_index = source_chunk, source_index

    def positions_tsv(self, name) -> str:
        """A '# name' line, then one line per base: index, letter, position (three decimals, 'nan' where unknown), Phred value;
        tab-separated.  Needs a result of basecall(..., moves=True)."""
        if self.positions is None:
            raise ValueError("positions_tsv needs basecall(..., moves=True)")
        rows = [f"{i}\t{c}\t{p:.3f}\t{int(q)}" for i, (c, p, q) in enumerate(zip(self.seq, self.positions, self.qualities))]
        return "\n".join([f"# {name}"] + rows) + "\n"

    def to_fastq(self, name) -> str:
        """Four lines: @name, the sequence, +, the qualities as chr(33 + Q)."""
        return f"@{name}\n{self.seq}\n+\n{(self.qualities + 33).astype(np.uint8).tobytes().decode('ascii')}\n"


class ReadHandle:
    """A read on the device (Basecaller.put_read): `read_id` for the first column of a window table, `drop()` when done."""

    def __init__(self, basecaller, read_id, n_raw, n_event, keep=None, windows=None):
        self._bc, self.read_id, self.n_raw, self.n_event, self._keep = basecaller, int(read_id), n_raw, n_event, keep
        self.windows = windows      # i32 [n,4], the read's own window table: set by Basecaller.put_signal(s), else None

    def fetch(self, what: str) -> np.ndarray:
        """A table of the read, copied back (rv_read_fetch): 'windows' i32 [n,4], 'raw_sc' f32 [N], 'events_sc' f32 [E,5], and of a
        read put from its signal 'start' / 'length' i64 [E], 'mean' / 'stdv' f64 [E]."""
        code, dtype, shape = {"windows": (_capi.RV_FETCH_WINDOWS, np.int32, (len(self.windows) if self.windows is not None else 0, 4)),
                              "raw_sc": (_capi.RV_FETCH_RAW_SC, np.float32, (self.n_raw,)),
                              "events_sc": (_capi.RV_FETCH_EVENTS_SC, np.float32, (self.n_event, 5)),
                              "start": (_capi.RV_FETCH_EVENT_START, np.int64, (self.n_event,)),
                              "length": (_capi.RV_FETCH_EVENT_LENGTH, np.int64, (self.n_event,)),
                              "mean": (_capi.RV_FETCH_EVENT_MEAN, np.float64, (self.n_event,)),
                              "stdv": (_capi.RV_FETCH_EVENT_STDV, np.float64, (self.n_event,))}[what]
        out = np.empty(shape, dtype)
        self._bc._check(self._bc._lib.rv_read_fetch(self._bc._h, self.read_id, code, out.ctypes.data_as(ctypes.c_void_p), out.nbytes),
                        "rv_read_fetch")
        return out

    def table(self, windows) -> np.ndarray:
        """windows i32 [n,4] (data_loader.prepare_windows) -> the [n,5] table of the window calls, this read's id in column 0."""
        w = np.asarray(windows, np.int32).reshape(-1, 4)
        return np.ascontiguousarray(np.column_stack((np.full(w.shape[0], self.read_id, np.int32), w)).astype(np.int32))

    def drop(self):
        """rv_read_drop; fails (RV_ESTATE) while an uncollected ticket uses the read.  A second drop does nothing."""
        if self.read_id >= 0:
            self._bc._check(self._bc._lib.rv_read_drop(self._bc._h, self.read_id), "rv_read_drop")
            self.read_id, self._keep = -1, None


def _as_int(x) -> int:
    """max_output_len arrives as tf.shape(target)[1] in the reference (a 0-d tensor)."""
    if isinstance(x, torch.Tensor):
        return int(x.item())
    return int(np.asarray(x).reshape(()))


class Basecaller:
    def __init__(self, enc_units: int, dec_units: int, batch_sz: int, tokenizer, input_data_type: str,
                 input_padding_value, encoder_depth: int = 2, decoder_depth: int = 1,
                 rnn_type: str = "bilstm", teacher_forcing=True, attention_type: str = "luong",
                 beam_width: int = 5, *, device: int | None = None, max_batch: int = 1024,
                 max_raw_len: int = 300, max_event_len: int = 45, max_output_len: int = 64,
                 honor_attention_type: bool = False, max_beam: int = 8):
        """Positional / keyword arguments are those of the reference constructor
        (basecaller.py:158).  Keyword-only extras size device memory (``max_beam``: the widest beam
        the handle will be asked for, 1..8).

        ``rnn_type``: 'bilstm' (BiLSTM encoders, LSTM decoder cells) or 'bigru' (BiGRU encoders, GRU decoder cells; Keras GRUCell
        defaults, DESIGN.md section 15 -- served on the per-step decode).  'lstm' and 'gru' raise NotImplementedError.

        The reference hard-codes Luong attention when it builds its Decoder
        (basecaller.py:194) and only stores ``attention_type`` (:201); that behaviour is kept
        unless ``honor_attention_type=True`` selects the Bahdanau mechanism that
        ``Decoder(attention_type='bahdanau')`` builds (basecaller.py:131-132)."""
        if rnn_type not in ("bilstm", "bigru"):
            raise NotImplementedError(
                f"rnn_type={rnn_type!r}: the bidirectional families are built ('bilstm': BiLSTM encoder / LSTM decoder; 'bigru': "
                f"BiGRU encoder / GRU decoder), the unidirectional ones are not")
        if input_data_type not in ("raw", "event", "joint"):
            raise ValueError(f"input_data_type {input_data_type!r}")
        self.batch_sz = batch_sz
        self.rnn_type = rnn_type
        self.tokenizer = tokenizer
        self.teacher_forcing = teacher_forcing
        self.input_data_type = input_data_type
        self.input_padding_value = input_padding_value
        self.attention_type = attention_type
        self.beam_width = beam_width
        self.max_input_len = {"raw": 200, "event": 30, "joint": 230}[input_data_type]   # basecaller.py:180-185
        self.output_start_token = np.int32(tokenizer.word_index["$"])
        self.output_end_token = np.int32(tokenizer.word_index["^"])
        self.output_padding_token = np.int32(tokenizer.word_index[""])

        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        self.cfg = RvConfig(
            enc_units=enc_units, dec_units=dec_units, enc_depth=encoder_depth, dec_depth=decoder_depth,
            mode=input_data_type,
            attention=attention_type if honor_attention_type else "luong",
            vocab=len(set(tokenizer.word_index.values())),      # = len(word_index) unless two of '' ^ $ share an id
            start_token=int(self.output_start_token), end_token=int(self.output_end_token),
            pad_token=int(self.output_padding_token), padding_value=float(input_padding_value),
            max_batch=max_batch, max_raw_len=max_raw_len, max_event_len=max_event_len,
            max_output_len=max_output_len, max_beam=int(max_beam), device=device, rnn=rnn_type)
        self.device = torch.device("cuda", device)
        self._lib = _capi.load_library()
        self._h = self._create_handle()
        self.optimizer = None
        self._weight_parts = 2

    # ------------------------------------------------------------------ lifecycle
    def _create_handle(self):
        """A handle of this configuration's cell family: rv_create for the BiLSTM, rv_create_rnn for every other one."""
        h = ctypes.c_void_p()
        ccfg = self.cfg.to_c()
        if self.cfg.rnn == "bilstm":
            rc, what = self._lib.rv_create(ctypes.byref(ccfg), ctypes.byref(h)), "rv_create"
        else:
            rc, what = self._lib.rv_create_rnn(ctypes.byref(ccfg), RNNS[self.cfg.rnn], ctypes.byref(h)), "rv_create_rnn"
        _capi.check(self._lib, None, rc, what)
        return h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.rv_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def compile(self, optimizer=None, **kwargs):
        """Keras ``compile`` (ravvent_performance_evaluator.py:104): inference needs no
        optimizer; accepted and ignored."""
        self.optimizer = optimizer

    def _check(self, rc, what):
        _capi.check(self._lib, self._h, rc, what)

    # ------------------------------------------------------------------ weights
    def set_weights_flat(self, flat: dict):
        blob = _weights.pack(self.cfg, flat)
        self._check(self._lib.rv_load_weights(self._h, blob.ctypes.data_as(ctypes.c_void_p), blob.size),
                    "rv_load_weights")
        self._blob = blob
        self._parts_loaded = self.weight_parts       # the mode the images in force were built in

    def clone(self):
        """A second handle on the same device with the same configuration and weights (own stream, own buffers): two handles
        driven from two host threads keep the GPU fed across slab boundaries (evaluator.PerformanceEvaluator(concurrent_slabs=2))."""
        other = object.__new__(Basecaller)
        for k, v in self.__dict__.items():
            if k not in ("_h", "_outs"):
                setattr(other, k, v)
        other._h = self._create_handle()
        # the mode travels with the clone: its images are built in the mode this handle's were LOADED in, and its option then says
        # what this handle's option says (the two differ after set_option("weight_parts", n) without a reload)
        loaded = getattr(self, "_parts_loaded", 2)
        if getattr(self, "_blob", None) is not None:
            if loaded != 2:
                other._check(self._lib.rv_set_option(other._h, b"weight_parts", loaded), "rv_set_option(weight_parts)")
            other._check(self._lib.rv_load_weights(other._h, self._blob.ctypes.data_as(ctypes.c_void_p), self._blob.size),
                         "rv_load_weights")
        if self.weight_parts != (loaded if getattr(self, "_blob", None) is not None else 2):
            other._check(self._lib.rv_set_option(other._h, b"weight_parts", self.weight_parts), "rv_set_option(weight_parts)")
        if self.gru_persistent:
            other._check(self._lib.rv_set_option(other._h, b"gru_persistent", 1), "rv_set_option(gru_persistent)")
        return other

    @property
    def weight_parts(self) -> int:
        """f16 parts each dense weight keeps (option ``weight_parts``, as set: in force from the next load of weights): 2 = fp32-exact
        weights, 1 = the half-precision weight mode.  ``weight_parts_loaded`` is the mode the weights in force were loaded in."""
        return getattr(self, "_weight_parts", 2)

    @property
    def weight_parts_loaded(self) -> int:
        return getattr(self, "_parts_loaded", 2)

    def set_weight_parts(self, n: int):
        """2 (default): every dense weight enters the matrix pipe as two f16 parts.  1: every such weight is rounded to its first
        part (include/ravvent_hip.h, option ``weight_parts``) -- a model with slightly other weights, decoded
        with half the weight stream.  Weights already loaded are loaded again from the kept blob, so the mode is in force when this
        returns.  Fails while asynchronous calls are in flight."""
        self._check(self._lib.rv_set_option(self._h, b"weight_parts", int(n)), "rv_set_option(weight_parts)")
        self._weight_parts = int(n)
        if getattr(self, "_blob", None) is not None:
            self._check(self._lib.rv_load_weights(self._h, self._blob.ctypes.data_as(ctypes.c_void_p), self._blob.size),
                        "rv_load_weights")
            self._parts_loaded = int(n)          # (only once the reload has succeeded)
        return self

    @property
    def gru_persistent(self) -> bool:
        """Whether option ``gru_persistent`` is on (``set_gru_persistent``)."""
        return bool(getattr(self, "_gru_persistent", False))

    def set_gru_persistent(self, on: bool = True):
        """A ``rnn_type='bigru'`` model of one decoder cell: decode every call in ONE launch of the persistent GRU kernel
        (``k_dec_persist_gru``) instead of two launches per output step (include/ravvent_hip.h, option ``gru_persistent``; DESIGN.md
        section 15).  Off by default.  The folded GRU images are built from the weights in force when this returns (else at the next
        load); turning it off returns to the per-step decode and frees nothing.  Fails on a BiLSTM model, with more than one decoder
        cell, and while asynchronous calls are in flight."""
        self._check(self._lib.rv_set_option(self._h, b"gru_persistent", int(bool(on))), "rv_set_option(gru_persistent)")
        self._gru_persistent = bool(on)
        return self

    def load_weights(self, path):
        """ravvent_performance_evaluator.py:107.  `path` is either a TF-format checkpoint prefix as Keras writes it
        (`prefix.index` + `prefix.data-*`: read by checkpoint.py without TensorFlow, variables matched by their
        attribute paths, weights_manifest.json) or this build's own ``.npz`` weight file (weights.py)."""
        from . import checkpoint
        if checkpoint.is_tf_checkpoint(path):
            self.set_weights_flat(checkpoint.flat_from_checkpoint(str(path), self.cfg))
        else:
            self.set_weights_flat(_weights.load(str(path), self.cfg))
        return self

    def init_random_weights(self, seed: int = 22, scheme: str = "keras", gain: float = 1.0):
        flat = _weights.init_weights(self.cfg, seed=seed, scheme=scheme, gain=gain)
        self.set_weights_flat(flat)
        return flat

    def set_option(self, key: str, value: int):
        rc = self._lib.rv_set_option(self._h, key.encode(), int(value))
        if rc > 0:      # a warning code (include/ravvent_hip.h): the option took effect, the message says what to look at
            import warnings
            msg = self._lib.rv_last_error(self._h)
            warnings.warn(f"rv_set_option({key}): {msg.decode() if msg else rc}", RuntimeWarning, stacklevel=2)
            return
        self._check(rc, f"rv_set_option({key})")
        if key == "weight_parts":
            self._weight_parts = int(value)
        if key == "gru_persistent":
            self._gru_persistent = bool(value)

    # ------------------------------------------------------------------ input plumbing
    def _split_inputs(self, input_data):
        if self.input_data_type == "joint":
            raw, ev = input_data
        elif self.input_data_type == "raw":
            raw, ev = input_data, None
        else:
            raw, ev = None, input_data
        return raw, ev

    def _prep(self, x, feat):
        """-> (keepalive, pointer, B, T, on_device)"""
        if x is None:
            return None, None, None, 0, None
        if isinstance(x, torch.Tensor):
            if x.dim() != 3 or x.shape[-1] != feat:
                raise ValueError(f"expected [B,T,{feat}], got {tuple(x.shape)}")
            if x.is_cuda:
                if x.device != self.device:
                    raise ValueError(f"input on {x.device}, basecaller on {self.device}")
                # (the usual case costs nothing: a submit's host time is what the GPU waits for when the queue runs low)
                t = x if (x.dtype == torch.float32 and x.is_contiguous() and not x.requires_grad) else x.detach().to(torch.float32).contiguous()
                return t, ctypes.c_void_p(t.data_ptr()), t.shape[0], t.shape[1], True
            x = x.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(x), dtype=np.float32)
        if a.ndim != 3 or a.shape[-1] != feat:
            raise ValueError(f"expected [B,T,{feat}], got {a.shape}")
        return a, a.ctypes.data_as(ctypes.c_void_p), a.shape[0], a.shape[1], False

    def _gather_inputs(self, input_data):
        raw, ev = self._split_inputs(input_data)
        kr, pr, Br, Tr, dr = self._prep(raw, RAW_FEATURES)
        ke, pe, Be, Te, de = self._prep(ev, EVENT_FEATURES)
        if kr is not None and ke is not None:
            if Br != Be:
                raise ValueError(f"raw batch {Br} != event batch {Be}")
            if dr != de:   # mixed residency: bring both to the host path
                if dr:
                    return self._gather_inputs((kr.cpu(), ke))
                return self._gather_inputs((kr, ke.cpu()))
        B = Br if kr is not None else Be
        on_dev = dr if kr is not None else de
        return (kr, ke), pr, pe, B, Tr, Te, on_dev

    # ------------------------------------------------------------------ the hot path
    def beam_search_prediction(self, input_data, beam_width, max_output_len):
        """basecaller.py:296-315 -> (predicted_ids[:,:,0] [B,S] int32, scores[:,:,0] [B,S] f32)."""
        keep, pr, pe, B, Tr, Te, on_dev = self._gather_inputs(input_data)
        L, W = _as_int(max_output_len), int(beam_width)
        steps = max(L - 1, 0)
        S = ctypes.c_int32(0)
        if on_dev:
            torch.cuda.current_stream(self.device).synchronize()   # inputs ready before the library's stream reads them
            tokens, scores = self._out_buffers("beam", B, steps, 1)
            rc = self._lib.rv_beam_search_dev(self._h, pr, pe, B, Tr, Te, W, L,
                                              ctypes.c_void_p(tokens.data_ptr()), ctypes.c_void_p(scores.data_ptr()),
                                              ctypes.byref(S))
        else:
            tk = np.empty((B, steps), np.int32)
            sc = np.empty((B, steps), np.float32)
            rc = self._lib.rv_beam_search(self._h, pr, pe, B, Tr, Te, W, L,
                                          tk.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p),
                                          ctypes.byref(S))
            tokens, scores = torch.from_numpy(tk), torch.from_numpy(sc)
        self._check(rc, "rv_beam_search")
        self.last_steps = S.value
        return tokens[:, :S.value], scores[:, :S.value]

    # ------------------------------------------------------------------ the whole beam
    def _beams_dev(self, B, steps, W):
        i32, f32 = torch.int32, torch.float32
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        return BeamHypotheses(mk((B, steps, W), i32), mk((B, steps, W), f32), mk((B, steps, W), f32), mk((B, W), f32), mk((B, W), i32))

    @staticmethod
    def _beams_host(B, steps, W):
        return BeamHypotheses(np.empty((B, steps, W), np.int32), np.empty((B, steps, W), np.float32), np.empty((B, steps, W), np.float32),
                              np.empty((B, W), np.float32), np.empty((B, W), np.int32))

    @staticmethod
    def _beams_struct(bufs):
        ptr = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)
        return _capi.CRvBeams(*[ptr(a) for a in bufs])

    @staticmethod
    def _beams_cut(bufs, S):
        t = [a if isinstance(a, torch.Tensor) else torch.from_numpy(a) for a in bufs]
        return BeamHypotheses(t[0][:, :S], t[1][:, :S], t[2][:, :S], t[3], t[4])

    def _check_beams_out(self, out, B, steps, W):
        want = (((B, steps, W), torch.int32), ((B, steps, W), torch.float32), ((B, steps, W), torch.float32), ((B, W), torch.float32),
                ((B, W), torch.int32))
        if len(out) != 5 or any(tuple(a.shape) != sh or a.dtype != dt or not a.is_contiguous() or a.device != self.device
                                for a, (sh, dt) in zip(out, want)):
            raise ValueError(f"out: five contiguous tensors on {self.device}: int32 / float32 / float32 {(B, steps, W)}, float32 / int32 {(B, W)}")
        return BeamHypotheses(*out)

    def beam_search_hypotheses(self, input_data, beam_width, max_output_len):
        """All `beam_width` hypotheses of every chunk (rv_beam_search_all / _all_dev): what tfa's BeamSearchDecoder returns before
        basecaller.py:313-315 keeps slot 0 -> BeamHypotheses(tokens [B,S,W] int32, scores [B,S,W] f32, path_scores [B,S,W] f32,
        log_probs [B,W] f32, lengths [B,W] int32).  tokens[:, :, 0] / scores[:, :, 0] are `beam_search_prediction`'s results;
        `utils.calc_prob_path_scores(path_scores)` gives each hypothesis's per-base probabilities."""
        keep, pr, pe, B, Tr, Te, on_dev = self._gather_inputs(input_data)
        L, W = _as_int(max_output_len), int(beam_width)
        steps = max(L - 1, 0)
        S = ctypes.c_int32(0)
        if on_dev:
            torch.cuda.current_stream(self.device).synchronize()   # inputs ready before the library's stream reads them
            bufs = self._beams_dev(B, steps, max(W, 0))
            st = self._beams_struct(bufs)
            rc = self._lib.rv_beam_search_all_dev(self._h, pr, pe, B, Tr, Te, W, L, ctypes.byref(st), ctypes.byref(S))
        else:
            bufs = self._beams_host(B, steps, max(W, 0))
            st = self._beams_struct(bufs)
            rc = self._lib.rv_beam_search_all(self._h, pr, pe, B, Tr, Te, W, L, ctypes.byref(st), ctypes.byref(S))
        self._check(rc, "rv_beam_search_all")
        self.last_steps = S.value
        return self._beams_cut(bufs, S.value)

    # ------------------------------------------------------------------ moves: where in the signal each called base lies
    def _moves_bufs(self, B, steps, W, on_dev):
        if on_dev:
            mk = lambda dt: torch.empty((B, steps, W), dtype=dt, device=self.device)
            f32, i32 = torch.float32, torch.int32
        else:
            mk = lambda dt: np.empty((B, steps, W), dt)
            f32, i32 = np.float32, np.int32
        return Moves(mk(f32), mk(f32), mk(f32), mk(f32), mk(i32), mk(f32))

    @staticmethod
    def _moves_struct(bufs):
        ptr = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)
        return _capi.CRvMoves(*[ptr(a) for a in bufs])

    @staticmethod
    def _moves_cut(bufs, S):
        return Moves(*[(a if isinstance(a, torch.Tensor) else torch.from_numpy(a))[:, :S] for a in bufs])

    def beam_search_moves(self, input_data, beam_width, max_output_len):
        """`beam_search_hypotheses` with the position of every token in the chunk's signal (rv_beam_search_moves / _moves_dev) ->
        (BeamHypotheses, Moves).  Moves: six [B,S,W] tensors -- raw_pos / event_pos f32: the attention-weighted mean sample / event
        index of the step that produced tokens[b, t, w] (-1 where that segment carries no weight), raw_mass / event_mass f32: the
        weight on each segment, peak int32 / peak_weight f32: the memory index (raw samples first, then events) of the largest
        weight.  Columns past a hypothesis's length hold -1 / 0.  Host or device tensors follow the inputs; the BeamHypotheses is
        `beam_search_hypotheses`'s byte for byte.  `base_positions` cuts a hypothesis's positions to its letters."""
        keep, pr, pe, B, Tr, Te, on_dev = self._gather_inputs(input_data)
        L, W = _as_int(max_output_len), int(beam_width)
        steps = max(L - 1, 0)
        S = ctypes.c_int32(0)
        if on_dev:
            torch.cuda.current_stream(self.device).synchronize()   # inputs ready before the library's stream reads them
            bufs = self._beams_dev(B, steps, max(W, 0))
        else:
            bufs = self._beams_host(B, steps, max(W, 0))
        mv = self._moves_bufs(B, steps, max(W, 0), on_dev)
        st, sm = self._beams_struct(bufs), self._moves_struct(mv)
        fn = self._lib.rv_beam_search_moves_dev if on_dev else self._lib.rv_beam_search_moves
        self._check(fn(self._h, pr, pe, B, Tr, Te, W, L, ctypes.byref(st), ctypes.byref(sm), ctypes.byref(S)), "rv_beam_search_moves")
        self.last_steps = S.value
        return self._beams_cut(bufs, S.value), self._moves_cut(mv, S.value)

    def base_positions(self, tokens, positions):
        """The positions of the letters of one hypothesis: `tokens` [B,S] (e.g. BeamHypotheses.tokens[:, :, w]) and `positions` [B,S]
        (the same slice of a Moves member) -> per chunk a 1-D array of the positions at the columns whose token
        `tokens_to_nuc_sequences` keeps; element i belongs to letter i of that chunk's string."""
        as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        tokens, positions = as_np(tokens), as_np(positions)
        if tokens.ndim != 2 or positions.shape != tokens.shape:
            raise ValueError(f"tokens and positions: two [B,S] arrays of one shape, got {tokens.shape} and {positions.shape}")
        if self.tokenizer.word_index == nuc_tk.word_index:       # the table tokens_to_nuc_sequences maps through: 0 = dropped
            table = _ASCII
        else:
            table = np.zeros(256, np.uint8)
            table[:8] = self._call_lut()
        kept = table[np.clip(tokens, 0, 255).astype(np.uint8)] != 0
        return [positions[b][kept[b]] for b in range(tokens.shape[0])]

    def label_positions(self, target_tokens, positions):
        """`base_positions` for a forced decode (`align`): `target_tokens` [B,L] and `positions` [B,L-1] (a Moves member of `align`) ->
        per chunk the positions at the columns whose label target_tokens[b, t+1] is a letter; element i belongs to letter i of the
        chunk's label string."""
        as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        return self.base_positions(as_np(target_tokens)[:, 1:], positions)

    # ------------------------------------------------------------------ the hot path, several slabs in flight
    def set_async_depth(self, depth: int):
        """Slab contexts the submit_* calls rotate through (1..16; default 2).  With several slabs in flight the GPU never idles
        at a slab boundary, and the encoder recurrences run 16 chunks per workgroup on the matrix pipe (option wide_recurrence)."""
        self.set_option("async_depth", int(depth))
        self.async_depth = int(depth)

    def set_coalesce(self, n: int):
        """Slabs of the submit_* calls decoded as one internal call (option coalesce): 0 / 1 none, 2..8 that many, -1 (default) chosen
        from the asynchronous depth.  A slab may then wait for its group: until it is full, a ticket of it is collected, `flush()`, ..."""
        self.set_option("coalesce", int(n))

    def flush(self):
        """Launch the group of submitted slabs that is still filling (rv_beam_search_flush); nothing to do without one."""
        self._check(self._lib.rv_beam_search_flush(self._h), "rv_beam_search_flush")

    supports_out = True       # submit_beam_search / beam_search_stream take caller-provided device outputs

    def submit_beam_search(self, input_data, beam_width, max_output_len, out=None, out_ptrs=None, all_beams=False, moves=False):
        """Queue `beam_search_prediction(input_data, ...)` without waiting for the GPU (rv_beam_search_submit / _submit_dev);
        returns a ticket for `collect`.  Results are byte-identical to the synchronous call.  Device inputs must stay untouched
        until the ticket is collected (the ticket keeps them alive).  `out` (device inputs only): a pair of contiguous device
        tensors (int32 [B, L-1], float32 [B, L-1]) the library writes into instead of fresh ones -- e.g. views into a gather buffer.
        `out_ptrs` (device inputs only): the same as two raw device addresses (the caller vouches for room, type and lifetime; `collect`
        then returns only the step count) -- a loop that submits thousands of slabs into one buffer saves the per-slab tensor views.
        `all_beams`: queue `beam_search_hypotheses` instead (rv_beam_search_submit_all / _submit_all_dev); `out` is then its five
        device tensors (tokens, scores, path_scores [B, L-1, W], log_probs, lengths [B, W]) and `collect` returns a BeamHypotheses.
        Such a slab is never coalesced with others.  `moves` (host inputs only): queue `beam_search_moves` instead
        (rv_beam_search_submit_moves); `collect` returns its (BeamHypotheses, Moves)."""
        keep, pr, pe, B, Tr, Te, on_dev = self._gather_inputs(input_data)
        L, W = _as_int(max_output_len), int(beam_width)
        steps = max(L - 1, 0)
        t = ctypes.c_int32(-1)
        if moves:
            if on_dev or out is not None or out_ptrs is not None:
                raise ValueError("moves=True takes host inputs and returns host results")
            self._check(self._lib.rv_beam_search_submit_moves(self._h, pr, pe, B, Tr, Te, W, L, ctypes.byref(t)), "rv_beam_search_submit_moves")
            return {"kind": "moves_host", "keep": keep, "B": B, "steps": steps, "W": max(W, 0), "ticket": t.value}
        if all_beams:
            if out_ptrs is not None:
                raise ValueError("all_beams takes its outputs as tensors (out=)")
            call = {"kind": "all_dev" if on_dev else "all_host", "keep": keep, "B": B, "steps": steps, "W": max(W, 0)}
            if on_dev:
                torch.cuda.current_stream(self.device).synchronize()
                bufs = self._check_beams_out(out, B, steps, W) if out is not None else self._beams_dev(B, steps, max(W, 0))
                call["out"] = bufs
                st = self._beams_struct(bufs)
                rc = self._lib.rv_beam_search_submit_all_dev(self._h, pr, pe, B, Tr, Te, W, L, ctypes.byref(st), ctypes.byref(t))
            else:
                if out is not None:
                    raise ValueError("out= needs device inputs")
                rc = self._lib.rv_beam_search_submit_all(self._h, pr, pe, B, Tr, Te, W, L, ctypes.byref(t))
            self._check(rc, "rv_beam_search_submit_all")
            call["ticket"] = t.value
            return call
        call = {"kind": "dev" if on_dev else "host", "keep": keep, "B": B, "steps": steps}
        if on_dev:
            torch.cuda.current_stream(self.device).synchronize()
            if out_ptrs is not None:
                rc = self._lib.rv_beam_search_submit_dev(self._h, pr, pe, B, Tr, Te, W, L, ctypes.c_void_p(int(out_ptrs[0])),
                                                         ctypes.c_void_p(int(out_ptrs[1])), ctypes.byref(t))
                self._check(rc, "rv_beam_search_submit")
                call["kind"] = "dev_ptrs"; call["ticket"] = t.value
                return call
            if out is not None:
                tokens, scores = out
                if (tuple(tokens.shape) != (B, steps) or tuple(scores.shape) != (B, steps) or tokens.dtype != torch.int32 or
                        scores.dtype != torch.float32 or not tokens.is_contiguous() or not scores.is_contiguous() or
                        tokens.device != self.device or scores.device != self.device):
                    raise ValueError(f"out: contiguous int32 / float32 tensors of shape {(B, steps)} on {self.device}")
            else:
                both = torch.empty((2, B, steps), dtype=torch.int32, device=self.device)      # one allocation: tokens | score bits
                tokens, scores = both[0], both[1].view(torch.float32)
            call["out"] = (tokens, scores)
            rc = self._lib.rv_beam_search_submit_dev(self._h, pr, pe, B, Tr, Te, W, L, ctypes.c_void_p(tokens.data_ptr()),
                                                     ctypes.c_void_p(scores.data_ptr()), ctypes.byref(t))
        else:
            rc = self._lib.rv_beam_search_submit(self._h, pr, pe, B, Tr, Te, W, L, ctypes.byref(t))
        self._check(rc, "rv_beam_search_submit")
        call["ticket"] = t.value
        return call

    def collect(self, call):
        """Wait for a `submit_beam_search` ticket -> (predicted_ids[:,:,0] [B,S] int32, scores[:,:,0] [B,S] f32), or the
        BeamHypotheses of an `all_beams` ticket, or the (BeamHypotheses, Moves) of a `moves` ticket."""
        S = ctypes.c_int32(0)
        if call["kind"] == "moves_host":
            bufs = self._beams_host(call["B"], call["steps"], call["W"])
            mv = self._moves_bufs(call["B"], call["steps"], call["W"], False)
            st, sm = self._beams_struct(bufs), self._moves_struct(mv)
            self._check(self._lib.rv_beam_search_collect_moves(self._h, call["ticket"], ctypes.byref(st), ctypes.byref(sm), ctypes.byref(S)),
                        "rv_beam_search_collect_moves")
            call["keep"] = None
            self.last_steps = S.value
            return self._beams_cut(bufs, S.value), self._moves_cut(mv, S.value)
        if call["kind"] in ("all_dev", "all_host"):
            if call["kind"] == "all_dev":
                self._check(self._lib.rv_beam_search_collect_dev(self._h, call["ticket"], ctypes.byref(S)), "rv_beam_search_collect_dev")
                bufs = call["out"]
            else:
                bufs = self._beams_host(call["B"], call["steps"], call["W"])
                st = self._beams_struct(bufs)
                self._check(self._lib.rv_beam_search_collect_all(self._h, call["ticket"], ctypes.byref(st), ctypes.byref(S)),
                            "rv_beam_search_collect_all")
            call["keep"] = None
            self.last_steps = S.value
            return self._beams_cut(bufs, S.value)
        if call["kind"] == "dev_ptrs":     # results went to the caller's addresses: only the step count comes back
            self._check(self._lib.rv_beam_search_collect_dev(self._h, call["ticket"], ctypes.byref(S)), "rv_beam_search_collect_dev")
            call["keep"] = None
            self.last_steps = S.value
            return S.value
        if call["kind"] == "dev":
            self._check(self._lib.rv_beam_search_collect_dev(self._h, call["ticket"], ctypes.byref(S)), "rv_beam_search_collect_dev")
            tokens, scores = call["out"]
        elif call["kind"] == "host":
            tk = np.empty((call["B"], call["steps"]), np.int32)
            sc = np.empty((call["B"], call["steps"]), np.float32)
            self._check(self._lib.rv_beam_search_collect(self._h, call["ticket"], tk.ctypes.data_as(ctypes.c_void_p),
                                                         sc.ctypes.data_as(ctypes.c_void_p), ctypes.byref(S)), "rv_beam_search_collect")
            tokens, scores = torch.from_numpy(tk), torch.from_numpy(sc)
        else:
            raise ValueError("collect_calls() takes the tickets of submit_calls()")
        call["keep"] = None
        self.last_steps = S.value
        return tokens[:, :S.value], scores[:, :S.value]

    def _call_lut(self):
        lut = np.zeros(8, np.uint8)
        for idx, word in self.tokenizer.index_word.items():
            if 0 <= idx < 8 and word not in ("", "^", "$", " "):
                lut[idx] = ord(word.upper())
        return lut

    def submit_calls(self, input_data, beam_width, max_output_len):
        """Asynchronous `beam_search_call_arrays` (rv_beam_search_submit_calls): host inputs, fused on-device post-processing."""
        keep, pr, pe, B, Tr, Te, on_dev = self._gather_inputs(input_data)
        if on_dev:
            host = tuple(None if k is None else k.cpu().numpy() for k in keep)
            return self.submit_calls(host if self.input_data_type == "joint" else (host[0] if host[0] is not None else host[1]),
                                     beam_width, max_output_len)
        L = _as_int(max_output_len)
        t = ctypes.c_int32(-1)
        lut = self._call_lut()
        self._check(self._lib.rv_beam_search_submit_calls(self._h, pr, pe, B, Tr, Te, int(beam_width), L,
                                                          lut.ctypes.data_as(ctypes.c_void_p), ctypes.byref(t)), "rv_beam_search_submit_calls")
        return {"kind": "calls", "ticket": t.value, "B": B, "steps": max(L - 1, 0)}

    def collect_calls(self, call):
        """-> (bases u8 [B, L-1], probs f32 [B, L-1], lengths i32 [B]) of a `submit_calls` ticket."""
        B, steps = call["B"], call["steps"]
        bases = np.zeros((B, steps), np.uint8); lens = np.zeros(B, np.int32); probs = np.zeros((B, steps), np.float32)
        S = ctypes.c_int32(0)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rv_beam_search_collect_calls(self._h, call["ticket"], p(bases), p(lens), p(probs), ctypes.byref(S)),
                    "rv_beam_search_collect_calls")
        self.last_steps = S.value
        return bases, probs, lens

    def beam_search_stream(self, slabs, beam_width, max_output_len, calls: bool = False, outs=None):
        """Generator: decode an iterable of slabs with `async_depth` of them in flight, yielding each slab's result in order
        ((tokens, scores), or (bases, probs, lengths) with calls=True) -- the overlapped form of a loop over
        `beam_search_prediction` / `beam_search_call_arrays`, with identical results."""
        depth = getattr(self, "async_depth", 2)
        outs = iter(outs) if outs is not None else None
        sub = self.submit_calls if calls else self.submit_beam_search
        col = self.collect_calls if calls else self.collect
        queue = []
        try:
            for x in slabs:
                if len(queue) >= depth:
                    yield col(queue.pop(0))
                if outs is not None:       # device inputs: the caller's output tensors, one pair per slab (submit_beam_search's `out`)
                    queue.append(sub(x, beam_width, max_output_len, out=next(outs)))
                else:
                    queue.append(sub(x, beam_width, max_output_len))
            while queue:
                yield col(queue.pop(0))
        finally:                       # a consumer that stops early (or an error): no ticket may stay uncollected on the handle
            while queue:
                try:
                    col(queue.pop(0))
                except Exception:
                    pass

    # ------------------------------------------------------------------ reads on the device, chunks as windows of them
    def put_read(self, raw_sc, events_sc, event_starts=None, event_lengths=None):
        """Upload a read's scaled tables once (rv_read_put; torch device tensors: rv_read_put_dev, no copy) -> ReadHandle.
        raw_sc f32 [N] (None in event mode), events_sc f32 [E,5] (None in raw mode): `data_loader.prepare_windows` makes both.
        The handle's `table(windows)` turns that function's [n,4] windows into the [n,5] tables the window calls take.
        event_starts / event_lengths (both or neither): the read's events as int64 [E], which a stitch by signal position needs in
        event and joint mode (rv_read_put_events)."""
        use_raw, use_ev = self.input_data_type != "event", self.input_data_type != "raw"
        on_dev = any(isinstance(x, torch.Tensor) and x.is_cuda for x in (raw_sc, events_sc))

        def prep(x, shape):
            if x is None:
                return None
            if on_dev:
                return torch.as_tensor(x).detach().to(device=self.device, dtype=torch.float32).reshape(shape).contiguous()
            x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
            return np.ascontiguousarray(np.asarray(x, np.float32).reshape(shape))
        r = prep(raw_sc, (-1,)) if use_raw else None
        e = prep(events_sc, (-1, 5)) if use_ev else None
        if (use_raw and r is None) or (use_ev and e is None):
            raise ValueError(f"{self.input_data_type} mode needs " + ("raw_sc" if use_raw and r is None else "events_sc"))
        ptr = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr() if on_dev else a.ctypes.data)
        n_raw, n_ev = (0 if r is None else int(r.shape[0])), (0 if e is None else int(e.shape[0]))
        rid = ctypes.c_int32(-1)
        if on_dev:
            torch.cuda.current_stream(self.device).synchronize()   # the tables are complete before the library's streams read them
            self._check(self._lib.rv_read_put_dev(self._h, ptr(r), n_raw, ptr(e), n_ev, ctypes.byref(rid)), "rv_read_put_dev")
        else:
            self._check(self._lib.rv_read_put(self._h, ptr(r), n_raw, ptr(e), n_ev, ctypes.byref(rid)), "rv_read_put")
        handle = ReadHandle(self, rid.value, n_raw, n_ev, (r, e) if on_dev else None)
        if event_starts is not None or event_lengths is not None:
            try:
                if event_starts is None or event_lengths is None:
                    raise ValueError("event_starts and event_lengths go together")
                st = np.ascontiguousarray(np.asarray(event_starts, np.int64).reshape(-1))
                ln = np.ascontiguousarray(np.asarray(event_lengths, np.int64).reshape(-1))
                if st.shape != ln.shape:
                    raise ValueError(f"event_starts {st.shape} and event_lengths {ln.shape} differ in length")
                self._check(self._lib.rv_read_put_events(self._h, handle.read_id, st.ctypes.data_as(ctypes.c_void_p),
                                                         ln.ctypes.data_as(ctypes.c_void_p), int(st.shape[0])), "rv_read_put_events")
            except Exception:
                handle.drop()
                raise
        return handle

    @staticmethod
    def _signal_int16(signal) -> np.ndarray:
        """A signal as the device path takes it: integer ADC counts that fit int16.  Anything else is refused, never rounded."""
        x = np.asarray(signal)
        if x.ndim != 1:
            x = x.reshape(-1)
        if x.dtype == np.int16:
            return np.ascontiguousarray(x)
        if x.dtype.kind not in "iuf" or (x.dtype.kind == "f" and not (np.isfinite(x).all() and (x == np.rint(x)).all())):
            raise ValueError("device preparation takes integer ADC samples; this signal is not integer-valued: use the host path "
                             "(basecall(..., device_prep=False), data_loader.prepare_windows)")
        if x.size and (x.min() < -32768 or x.max() > 32767):
            raise ValueError("device preparation takes samples that fit int16; this signal does not: use the host path "
                             "(basecall(..., device_prep=False), data_loader.prepare_windows)")
        return np.ascontiguousarray(x.astype(np.int16))

    def put_signals(self, signals, stride=6, max_raw_len=None, max_event_len=None, detector=None):
        """Reads from their raw signals, prepared on the device (rv_read_put_signals): one upload of the int16 samples, then the
        events, both scaled tables and the window table of every read are made by kernels -> list of ReadHandle, each with
        `.windows` (i32 [n,4], what `data_loader.prepare_windows` gives for the unlabelled read) ready for `.table()`.
        detector: an `EventDetector` for other parameters than the chunker's (windows 6 / 9).  ValueError for a signal that is not
        integer-valued or does not fit int16."""
        from .event_detection import EventDetector
        xs = [self._signal_int16(sig) for sig in signals]
        R = len(xs)
        if R == 0:
            return []
        dp = (detector or EventDetector(window_length1=_dl.ED_WINDOW_LENGTH_1, window_length2=_dl.ED_WINDOW_LENGTH_2)).params
        T_r = min(_dl.MAX_RAW_LEN, self.cfg.max_raw_len) if max_raw_len is None else int(max_raw_len)
        T_e = min(_dl.MAX_EVENT_LEN, self.cfg.max_event_len) if max_event_len is None else int(max_event_len)
        prep = _capi.CRvSignalPrep(int(dp["window_length1"]), int(dp["window_length2"]), float(dp["threshold1"]), float(dp["threshold2"]),
                                   float(dp["peak_height"]), int(stride), T_r, T_e)
        ptrs = (ctypes.c_void_p * R)(*[x.ctypes.data if x.size else None for x in xs])
        lens = (ctypes.c_size_t * R)(*[int(x.size) for x in xs])
        ids, nev, nwin = np.full(R, -1, np.int32), np.zeros(R, np.int32), np.zeros(R, np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rv_read_put_signals(self._h, R, ptrs, lens, ctypes.byref(prep), p(ids), p(nev), p(nwin)), "rv_read_put_signals")
        handles = [ReadHandle(self, int(ids[r]), int(xs[r].size), int(nev[r])) for r in range(R)]
        try:
            for r, h in enumerate(handles):
                h.windows = np.empty((int(nwin[r]), 4), np.int32)
                if nwin[r]:
                    h.windows = h.fetch("windows")
        except Exception:
            for h in handles:
                h.drop()
            raise
        return handles

    def put_signal(self, signal, **kwargs):
        """`put_signals` of one read -> ReadHandle."""
        return self.put_signals([signal], **kwargs)[0]

    def _window_table(self, windows, T_r, T_e):
        w = np.ascontiguousarray(np.asarray(windows, np.int32))
        if w.ndim != 2 or w.shape[1] != 5:
            raise ValueError(f"windows: expected [B,5] (read_id, raw_start, raw_len, event_start, event_len), got {w.shape}")
        T_r = min(_dl.MAX_RAW_LEN, self.cfg.max_raw_len) if T_r is None else int(T_r)
        T_e = min(_dl.MAX_EVENT_LEN, self.cfg.max_event_len) if T_e is None else int(T_e)
        return w, w.ctypes.data_as(ctypes.c_void_p), int(w.shape[0]), T_r, T_e

    def beam_search_windows(self, windows, beam_width, max_output_len, *, T_r=None, T_e=None, device_outputs=False):
        """`beam_search_prediction` on chunks that are windows of reads put with `put_read` (rv_beam_search_windows / _dev):
        windows i32 [B,5] = (read_id, raw_start, raw_len, event_start, event_len); chunk b is its windows padded to T_r / T_e
        (default: the chunker's 200 / 30).  Byte-identical to the call on `data_loader.expand_windows` of the same rows."""
        w, pw, B, T_r, T_e = self._window_table(windows, T_r, T_e)
        L, W = _as_int(max_output_len), int(beam_width)
        steps = max(L - 1, 0)
        S = ctypes.c_int32(0)
        if device_outputs:
            tokens, scores = self._out_buffers("beam", B, steps, 1)
            rc = self._lib.rv_beam_search_windows_dev(self._h, pw, B, T_r, T_e, W, L, ctypes.c_void_p(tokens.data_ptr()),
                                                      ctypes.c_void_p(scores.data_ptr()), ctypes.byref(S))
        else:
            tk, sc = np.empty((B, steps), np.int32), np.empty((B, steps), np.float32)
            rc = self._lib.rv_beam_search_windows(self._h, pw, B, T_r, T_e, W, L, tk.ctypes.data_as(ctypes.c_void_p),
                                                  sc.ctypes.data_as(ctypes.c_void_p), ctypes.byref(S))
            tokens, scores = torch.from_numpy(tk), torch.from_numpy(sc)
        self._check(rc, "rv_beam_search_windows")
        self.last_steps = S.value
        return tokens[:, :S.value], scores[:, :S.value]

    def beam_search_windows_call_arrays(self, windows, beam_width, max_output_len, *, T_r=None, T_e=None):
        """`beam_search_call_arrays` on windows (rv_beam_search_windows_calls) -> (bases u8 [B,L-1], probs f32 [B,L-1], lengths i32 [B])."""
        w, pw, B, T_r, T_e = self._window_table(windows, T_r, T_e)
        L = _as_int(max_output_len)
        steps = max(L - 1, 0)
        lut = self._call_lut()
        bases = np.zeros((B, steps), np.uint8); lens = np.zeros(B, np.int32); probs = np.zeros((B, steps), np.float32)
        S = ctypes.c_int32(0)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rv_beam_search_windows_calls(self._h, pw, B, T_r, T_e, int(beam_width), L, p(lut), p(bases), p(lens),
                                                           p(probs), ctypes.byref(S)), "rv_beam_search_windows_calls")
        self.last_steps = S.value
        return bases, probs, lens

    @staticmethod
    def _call_moves_bufs(B, steps):
        f = lambda: np.zeros((B, steps), np.float32)
        return CallMoves(f(), f(), f(), f(), np.zeros((B, steps), np.int32), f())

    @staticmethod
    def _call_moves_struct(bufs):
        return _capi.CRvCallMoves(*[ctypes.c_void_p(a.ctypes.data) for a in bufs])

    def beam_search_calls_moves(self, input_data, beam_width, max_output_len):
        """`beam_search_call_arrays` with the position of every called letter (rv_beam_search_calls_moves) -> (bases u8 [B,L-1],
        probs f32 [B,L-1], lengths i32 [B], CallMoves of six [B,L-1] arrays).  The first three are `beam_search_call_arrays`'s byte
        for byte; element i < lengths[b] of a CallMoves member is what `base_positions` cuts from `beam_search_moves` for letter i of
        hypothesis 0, the tail holds -1 (positions, peak) / 0.  Host buffers: device inputs are brought down."""
        keep, pr, pe, B, Tr, Te, on_dev = self._gather_inputs(input_data)
        if on_dev:
            host = tuple(None if k is None else k.cpu().numpy() for k in keep)
            return self.beam_search_calls_moves(host if self.input_data_type == "joint" else (host[0] if host[0] is not None else host[1]),
                                                beam_width, max_output_len)
        L = _as_int(max_output_len)
        steps = max(L - 1, 0)
        lut = self._call_lut()
        bases = np.zeros((B, steps), np.uint8); lens = np.zeros(B, np.int32); probs = np.zeros((B, steps), np.float32)
        mv = self._call_moves_bufs(B, steps)
        sm = self._call_moves_struct(mv)
        S = ctypes.c_int32(0)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rv_beam_search_calls_moves(self._h, pr, pe, B, Tr, Te, int(beam_width), L, p(lut), p(bases), p(lens),
                                                         p(probs), ctypes.byref(sm), ctypes.byref(S)), "rv_beam_search_calls_moves")
        self.last_steps = S.value
        return bases, probs, lens, mv

    def beam_search_windows_calls_moves(self, windows, beam_width, max_output_len, *, T_r=None, T_e=None):
        """`beam_search_calls_moves` on windows (rv_beam_search_windows_calls_moves): positions in samples / events of each CHUNK."""
        w, pw, B, T_r, T_e = self._window_table(windows, T_r, T_e)
        L = _as_int(max_output_len)
        steps = max(L - 1, 0)
        lut = self._call_lut()
        bases = np.zeros((B, steps), np.uint8); lens = np.zeros(B, np.int32); probs = np.zeros((B, steps), np.float32)
        mv = self._call_moves_bufs(B, steps)
        sm = self._call_moves_struct(mv)
        S = ctypes.c_int32(0)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rv_beam_search_windows_calls_moves(self._h, pw, B, T_r, T_e, int(beam_width), L, p(lut), p(bases), p(lens),
                                                                 p(probs), ctypes.byref(sm), ctypes.byref(S)),
                    "rv_beam_search_windows_calls_moves")
        self.last_steps = S.value
        return bases, probs, lens, mv

    def collect_calls_moves(self, call):
        """-> (bases, probs, lengths, CallMoves) of a `submit_windows(..., calls=True, moves=True)` ticket."""
        B, steps = call["B"], call["steps"]
        bases = np.zeros((B, steps), np.uint8); lens = np.zeros(B, np.int32); probs = np.zeros((B, steps), np.float32)
        mv = self._call_moves_bufs(B, steps)
        sm = self._call_moves_struct(mv)
        S = ctypes.c_int32(0)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rv_beam_search_collect_calls_moves(self._h, call["ticket"], p(bases), p(lens), p(probs), ctypes.byref(sm),
                                                                 ctypes.byref(S)), "rv_beam_search_collect_calls_moves")
        self.last_steps = S.value
        return bases, probs, lens, mv

    def submit_windows(self, windows, beam_width, max_output_len, calls=False, *, T_r=None, T_e=None, moves=False):
        """Queue `beam_search_windows` (calls=True: with the fused post-processing) without waiting for the GPU
        (rv_beam_search_submit_windows / _windows_calls); the ticket goes to `collect` / `collect_calls`.  The reads the table
        names cannot be dropped until the ticket is collected.  moves=True (with calls): `beam_search_windows_calls_moves`
        (rv_beam_search_submit_windows_calls_moves); the ticket goes to `collect_calls_moves`."""
        w, pw, B, T_r, T_e = self._window_table(windows, T_r, T_e)
        L = _as_int(max_output_len)
        t = ctypes.c_int32(-1)
        if moves:
            if not calls:
                raise ValueError("moves=True goes with calls=True")
            lut = self._call_lut()
            self._check(self._lib.rv_beam_search_submit_windows_calls_moves(self._h, pw, B, T_r, T_e, int(beam_width), L,
                                                                            lut.ctypes.data_as(ctypes.c_void_p), ctypes.byref(t)),
                        "rv_beam_search_submit_windows_calls_moves")
            return {"kind": "calls_moves", "ticket": t.value, "B": B, "steps": max(L - 1, 0)}
        if calls:
            lut = self._call_lut()
            self._check(self._lib.rv_beam_search_submit_windows_calls(self._h, pw, B, T_r, T_e, int(beam_width), L,
                                                                      lut.ctypes.data_as(ctypes.c_void_p), ctypes.byref(t)),
                        "rv_beam_search_submit_windows_calls")
            return {"kind": "calls", "ticket": t.value, "B": B, "steps": max(L - 1, 0)}
        self._check(self._lib.rv_beam_search_submit_windows(self._h, pw, B, T_r, T_e, int(beam_width), L, ctypes.byref(t)),
                    "rv_beam_search_submit_windows")
        return {"kind": "host", "keep": None, "ticket": t.value, "B": B, "steps": max(L - 1, 0)}

    def beam_search_stream_windows(self, tables, beam_width, max_output_len, calls: bool = False, *, T_r=None, T_e=None, moves=False):
        """`beam_search_stream` over window tables: `async_depth` slabs in flight, each table's result in order."""
        depth = getattr(self, "async_depth", 2)
        col = self.collect_calls_moves if moves else (self.collect_calls if calls else self.collect)
        queue = []
        try:
            for w in tables:
                if len(queue) >= depth:
                    yield col(queue.pop(0))
                if moves:
                    queue.append(self.submit_windows(w, beam_width, max_output_len, calls=True, T_r=T_r, T_e=T_e, moves=True))
                else:
                    queue.append(self.submit_windows(w, beam_width, max_output_len, calls=calls, T_r=T_r, T_e=T_e))
            while queue:
                yield col(queue.pop(0))
        finally:                       # (as beam_search_stream: no ticket may stay uncollected on the handle)
            while queue:
                try:
                    col(queue.pop(0))
                except Exception:
                    pass

    def _stream_window_calls(self, table, beam_width, L, chunk_size, T_r, T_e, moves=False):
        """The call arrays of a whole table, decoded in slabs of `chunk_size` rows with the handle's depth of them in flight.
        moves: through the calls-with-positions window call; a CallMoves over all rows comes fourth."""
        n, steps = int(table.shape[0]), max(L - 1, 0)
        bases = np.zeros((n, steps), np.uint8); probs = np.zeros((n, steps), np.float32); lens = np.zeros(n, np.int32)
        cuts = [(a, min(a + chunk_size, n)) for a in range(0, n, chunk_size)]
        if moves:
            mv = self._call_moves_bufs(n, steps)
            results = self.beam_search_stream_windows((table[a:b] for a, b in cuts), beam_width, L, calls=True, T_r=T_r, T_e=T_e, moves=True)
            for (a, b), (bs, pr, ln, m) in zip(cuts, results):
                bases[a:b] = bs; probs[a:b] = pr; lens[a:b] = ln
                for dst, src in zip(mv, m):
                    dst[a:b] = src
            return bases, probs, lens, mv
        results = self.beam_search_stream_windows((table[a:b] for a, b in cuts), beam_width, L, calls=True, T_r=T_r, T_e=T_e)
        for (a, b), (bs, pr, ln) in zip(cuts, results):
            bases[a:b] = bs; probs[a:b] = pr; lens[a:b] = ln
        return bases, probs, lens

    # ------------------------------------------------------------------ stitching a read by signal position
    @staticmethod
    def _stitch_out(capacity, n_reads):
        """Host arrays for the outputs of a stitch and the struct that names them."""
        cap = max(int(capacity), 0)
        arrs = [np.empty(cap, np.uint8), np.empty(cap, np.float32), np.empty(cap, np.float64), np.empty(cap, np.float32),
                np.empty(cap, np.float32), np.empty(cap, np.int32), np.empty(cap, np.int32), np.zeros(n_reads + 1, np.int64)]
        ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
        return arrs, _capi.CRvStitchOut(*[ptr(a) for a in arrs[:7]], cap, ptr(arrs[7]))

    @staticmethod
    def _stitch_cut(arrs):
        total = int(arrs[7][-1])
        return StitchedCalls(*[a[:total] for a in arrs[:7]], arrs[7])

    def stitch_calls(self, bases, probs, lengths, moves, windows, read_rows, capacity=None):
        """Stitch reads from their chunks' calls by signal position (rv_stitch_calls) -> StitchedCalls.
        bases u8 / probs f32 [n, stride] and lengths i32 [n] as the call-array calls return them, moves: a CallMoves (or any object
        with raw_pos / raw_mass / event_pos / event_mass [n, stride]), windows i32 [n,5] the table the calls ran on, read_rows
        [n_reads + 1] the first row of every read.  Each chunk owns the signal up to half way to its neighbours' centres, and keeps
        its bases from the first to the last one that lies there.  The reads of the table must be alive, and in event and joint mode
        hold their events (`put_signals`, or `put_read(..., event_starts=, event_lengths=)`).  capacity: elements the outputs
        hold (default: n x stride, which always suffices)."""
        c = lambda a, dt: np.ascontiguousarray(np.asarray(a), dtype=dt)
        bases, probs, lengths = c(bases, np.uint8), c(probs, np.float32), c(lengths, np.int32).reshape(-1)
        n = int(lengths.shape[0])
        if bases.ndim != 2 or bases.shape[0] != n or probs.shape != bases.shape:
            raise ValueError(f"bases and probs: two [{n},stride] arrays, got {bases.shape} and {probs.shape}")
        stride = int(bases.shape[1])
        mv = [c(getattr(moves, k), np.float32) for k in ("raw_pos", "raw_mass", "event_pos", "event_mass")]
        if any(m.shape != bases.shape for m in mv):
            raise ValueError(f"moves: four arrays of shape {bases.shape}")
        win = c(windows, np.int32)
        if win.shape != (n, 5):
            raise ValueError(f"windows: expected [{n},5] (read_id, raw_start, raw_len, event_start, event_len), got {win.shape}")
        rows = c(read_rows, np.int32).reshape(-1)
        if rows.shape[0] < 1:
            raise ValueError("read_rows: n_reads + 1 entries")
        ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
        cin = _capi.CRvStitchIn(ptr(bases), ptr(probs), ptr(lengths), *[ptr(m) for m in mv], ptr(win), n, stride)
        arrs, cout = self._stitch_out(n * stride if capacity is None else capacity, int(rows.shape[0]) - 1)
        self._check(self._lib.rv_stitch_calls(self._h, ctypes.byref(cin), int(rows.shape[0]) - 1, ptr(rows), ctypes.byref(cout)), "rv_stitch_calls")
        return self._stitch_cut(arrs)

    def _put_signals_for_calls(self, signals, stride, T_r, T_e, device_prep, events, handles, windows, ev_tabs):
        """The preparation `basecall_many` starts with, for either merge: every read on the device and its window table [n,4], by
        `put_signals` (device_prep) or read by read through `prepare_windows` and `put_read`.  The handles, windows and event
        tables (starts, lengths) are appended to the caller's lists as they come, so that its `finally` drops whatever was put.
        events None: no event tables; "host": in ev_tabs (fetched from a device-made read); "device": the reads hold them on the
        device -- those of `put_signals` do, a host-made read is given the host detector's arrays (rv_read_put_events)."""
        from .event_detection import EventDetector
        if device_prep:
            handles.extend(self.put_signals(list(signals), stride=stride, max_raw_len=T_r, max_event_len=T_e))
            windows.extend(h.windows for h in handles)
            if events == "host":      # the read's events, as the device made them
                ev_tabs.extend((h.fetch("start"), h.fetch("length")) if h.n_event else (np.zeros(0, np.int64), np.zeros(0, np.int64))
                               for h in handles)
            return
        for sig in signals:
            rw = _dl.prepare_windows(sig, stride=stride, max_raw_len=T_r, max_event_len=T_e)
            windows.append(rw.windows)
            if events is None:
                handles.append(self.put_read(rw.raw_sc, rw.events_sc))
                continue
            # ... as the host detector makes them: a second run of the detector prepare_windows ran, whose return type has no room
            # for the event arrays
            st, ln, _, _ = EventDetector(window_length1=_dl.ED_WINDOW_LENGTH_1, window_length2=_dl.ED_WINDOW_LENGTH_2).run_arrays(np.asarray(sig))
            st, ln = np.asarray(st, np.int64), np.asarray(ln, np.int64)
            if events == "host":
                handles.append(self.put_read(rw.raw_sc, rw.events_sc))
                ev_tabs.append((st, ln))
            else:
                handles.append(self.put_read(rw.raw_sc, rw.events_sc, event_starts=st, event_lengths=ln))

    def _basecall_many_position(self, signals, stride, beam_width, max_output_len, chunk_size, device_prep):
        """`basecall_many(..., merge="position")`: the slabs stream through the stitch submit into one device buffer, one
        rv_stitch_run follows, and the reads come back stitched -- no slab result is copied to the host, no alignment runs."""
        L = self.cfg.max_output_len if max_output_len is None else _as_int(max_output_len)
        T_r, T_e = min(_dl.MAX_RAW_LEN, self.cfg.max_raw_len), min(_dl.MAX_EVENT_LEN, self.cfg.max_event_len)
        windows, handles = [], []
        sb = ctypes.c_void_p()
        queue = []
        S = ctypes.c_int32(0)
        try:
            # (raw mode: the positions are the raw estimate, which reads no event table)
            self._put_signals_for_calls(signals, stride, T_r, T_e, device_prep, None if self.input_data_type == "raw" else "device",
                                        handles, windows, [])
            n = [int(w.shape[0]) for w in windows]
            rows = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
            table = (np.concatenate([h.table(w) for h, w in zip(handles, windows)]) if windows else np.zeros((0, 5), np.int32))
            total, steps = int(table.shape[0]), max(L - 1, 0)
            self._check(self._lib.rv_stitch_open(self._h, total, L, ctypes.byref(sb)), "rv_stitch_open")
            lut = self._call_lut()
            depth = getattr(self, "async_depth", 2)
            collect = lambda t: self._check(self._lib.rv_beam_search_collect_stitch(self._h, t, ctypes.byref(S)), "rv_beam_search_collect_stitch")
            for a in range(0, total, int(chunk_size)):
                if len(queue) >= depth:
                    collect(queue.pop(0))
                w = np.ascontiguousarray(table[a:a + int(chunk_size)])
                t = ctypes.c_int32(-1)
                self._check(self._lib.rv_beam_search_submit_windows_stitch(self._h, w.ctypes.data_as(ctypes.c_void_p), int(w.shape[0]), T_r, T_e,
                                                                           int(beam_width), L, lut.ctypes.data_as(ctypes.c_void_p), sb, a,
                                                                           ctypes.byref(t)), "rv_beam_search_submit_windows_stitch")
                queue.append(t.value)
            while queue:
                collect(queue.pop(0))
            self.last_steps = S.value
            arrs, cout = self._stitch_out(total * steps, len(windows))
            self._check(self._lib.rv_stitch_run(self._h, sb, len(windows), rows.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cout)), "rv_stitch_run")
        finally:
            while queue:                   # (an error: no ticket may stay uncollected on the handle)
                try:
                    collect(queue.pop(0))
                except Exception:
                    pass
            if sb:
                self._lib.rv_stitch_close(self._h, sb)
            for h in handles:
                h.drop()
        r = self._stitch_cut(arrs)
        flat = r.bases.tobytes()
        out = []
        for i in range(len(windows)):
            a, b = int(r.read_offsets[i]), int(r.read_offsets[i + 1])
            out.append(BasecallResult(flat[a:b].decode("ascii"), r.probs[a:b].copy(), n[i], r.positions[a:b].copy(), r.raw_mass[a:b].copy(),
                                      r.event_mass[a:b].copy(), r.source_chunk[a:b].copy(), r.source_index[a:b].copy()))
        return out

    def basecall(self, signal, stride=6, beam_width=5, max_output_len=None, chunk_size=1024, device_prep=False, moves=False, merge="align"):
        """An unlabelled read's signal -> BasecallResult (seq, probs, qualities, chunks_num, to_fastq): `prepare_windows` without
        labels, `put_read`, window slabs of `chunk_size` chunks streamed with the fused post-processing, the C++ merger, drop.
        max_output_len None: the handle's.  device_prep, moves, merge: see `basecall_many`."""
        return self.basecall_many([signal], stride, beam_width, max_output_len, chunk_size, device_prep, moves, merge)[0]

    def basecall_many(self, signals, stride=6, beam_width=5, max_output_len=None, chunk_size=1024, device_prep=False, moves=False,
                      merge="align"):
        """`basecall` of several reads through shared slabs: the windows of all reads are queued into full slabs (a slab's rows may
        name different reads) and each read is stitched from its own rows -> list of BasecallResult, equal to one `basecall` each.
        device_prep True: events, scaling and windows are made on the device from the int16 samples of all reads at once
        (`put_signals`) instead of read by read on the host; integer signals only (ValueError otherwise).
        moves True: the slabs stream through the calls-with-positions window call and the merger reports where each merged base
        came from; every result then carries positions / raw_mass / event_mass / source_chunk / source_index (BasecallResult,
        `signal_positions`).  seq and probs are what moves=False gives, byte for byte.
        merge "align" (default): the chunks' calls come to the host and the C++ merger chains one local alignment per chunk pair.
        "position": the reads are stitched on the device by signal position instead (every chunk keeps the
        bases that lie on its own stretch of signal; `stitch_calls` states the rule) -- another read than "align" gives, with every
        position field set whatever `moves` says; which of the two is the more accurate is not measured."""
        if merge != "align":
            if merge != "position":
                raise ValueError(f"merge {merge!r}: 'align' or 'position'")
            return self._basecall_many_position(signals, stride, beam_width, max_output_len, chunk_size, device_prep)
        from . import merger as _merger
        L = self.cfg.max_output_len if max_output_len is None else _as_int(max_output_len)
        T_r, T_e = min(_dl.MAX_RAW_LEN, self.cfg.max_raw_len), min(_dl.MAX_EVENT_LEN, self.cfg.max_event_len)
        windows, handles, ev_tabs = [], [], []
        mv = None
        try:
            self._put_signals_for_calls(signals, stride, T_r, T_e, device_prep, "host" if moves else None, handles, windows, ev_tabs)
            n = [int(w.shape[0]) for w in windows]
            off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
            table = (np.concatenate([h.table(w) for h, w in zip(handles, windows)]) if windows else np.zeros((0, 5), np.int32))
            if moves:
                bases, probs, lens, mv = self._stream_window_calls(table, beam_width, L, int(chunk_size), T_r, T_e, moves=True)
            else:
                bases, probs, lens = self._stream_window_calls(table, beam_width, L, int(chunk_size), T_r, T_e)
        finally:
            for h in handles:
                h.drop()
        mg = _merger.Merger()
        out = []
        for i in range(len(windows)):
            a, b = int(off[i]), int(off[i + 1])
            if not moves:
                seq, pr = mg.merge_arrays(bases[a:b], probs[a:b], lens[a:b]) if b > a else ("", np.zeros(0, np.float32))
                out.append(BasecallResult(seq, pr, n[i]))
                continue
            if b > a:
                seq, pr, ck, ix = mg.merge_arrays(bases[a:b], probs[a:b], lens[a:b], sources=True)
            else:
                seq, pr, ck, ix = "", np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32)
            # every per-base payload is a gather by the merger's (chunk, index) pairs; the scaled raw table starts at sample 0 of the
            # signal (prepare_windows scales the whole read), so no offset is added
            w = windows[i]
            g = lambda m: m[a:b][ck, ix]
            pos = signal_positions(self.input_data_type, w[ck, 0], w[ck, 2], g(mv.raw_pos), g(mv.raw_mass), g(mv.event_pos),
                                   g(mv.event_mass), ev_tabs[i][0], ev_tabs[i][1])
            out.append(BasecallResult(seq, pr, n[i], pos, g(mv.raw_mass).copy(), g(mv.event_mass).copy(), ck, ix))
        return out

    def greedy_search_prediction(self, input_data, max_output_len):
        """basecaller.py:317-330 -> (sample_id [B,S] int32, rnn_output logits [B,S,V] f32)."""
        keep, pr, pe, B, Tr, Te, on_dev = self._gather_inputs(input_data)
        L, V = _as_int(max_output_len), self.cfg.vocab
        steps = max(L - 1, 0)
        S = ctypes.c_int32(0)
        if on_dev:
            torch.cuda.current_stream(self.device).synchronize()
            tokens, logits = self._out_buffers("greedy", B, steps, V)
            rc = self._lib.rv_greedy_search_dev(self._h, pr, pe, B, Tr, Te, L,
                                                ctypes.c_void_p(tokens.data_ptr()), ctypes.c_void_p(logits.data_ptr()),
                                                ctypes.byref(S))
        else:
            tk = np.empty((B, steps), np.int32)
            lg = np.empty((B, steps, V), np.float32)
            rc = self._lib.rv_greedy_search(self._h, pr, pe, B, Tr, Te, L,
                                            tk.ctypes.data_as(ctypes.c_void_p), lg.ctypes.data_as(ctypes.c_void_p),
                                            ctypes.byref(S))
            tokens, logits = torch.from_numpy(tk), torch.from_numpy(lg)
        self._check(rc, "rv_greedy_search")
        self.last_steps = S.value
        return tokens[:, :S.value], logits[:, :S.value]

    # ------------------------------------------------------------------ scoring given label sequences
    def _omit_mask(self, tokens):
        """masked_accuracy's omit_vals (utils.py:15-24) as the bit mask over token ids the C-ABI takes."""
        m = 0
        for t in tokens:
            m |= 1 << int(t)
        return m

    @property
    def _train_omit(self):      # basecaller.py:247
        return (self.output_padding_token, self.output_start_token, self.output_end_token)

    @property
    def _val_omit(self):        # basecaller.py:277
        return (self.output_start_token, self.output_end_token)

    @staticmethod
    def _quotients(sc):
        """loss = sum(mask * loss) / sum(mask) in float32 (basecaller.py:218-219), acc = count / total in float64 (utils.py:22-24);
        NaN when nothing is counted, as the reference's divisions give."""
        t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
        loss = t(sc.nll_sum).sum(dtype=torch.float32) / t(sc.n_labels).sum().to(torch.float32)
        acc = t(sc.n_match).sum().to(torch.float64) / t(sc.n_counted).sum().to(torch.float64)
        return {"loss": loss.cpu(), "acc": acc.cpu()}

    def _teacher_forced(self, input_data, target_tokens, omit, moves=False):
        """One rv_teacher_forced / _dev call -> ForcedScores over the L - 1 positions of every chunk.  Host inputs take host labels
        (checked by the library: an id outside the vocabulary is RV_EINVAL); device inputs take the labels to the device unchecked
        (the kernels never index with such an id: it adds no input row, and as a label its nll is NaN).
        moves: rv_teacher_forced_moves / _dev -> (ForcedScores, Moves of six [B,L-1] tensors)."""
        keep, pr, pe, B, Tr, Te, on_dev = self._gather_inputs(input_data)
        V = self.cfg.vocab
        if isinstance(target_tokens, torch.Tensor) and not on_dev:
            target_tokens = target_tokens.detach().cpu().numpy()
        if on_dev:
            tg = torch.as_tensor(target_tokens).to(device=self.device, dtype=torch.int32).contiguous()
        else:
            tg = np.ascontiguousarray(np.asarray(target_tokens), dtype=np.int32)
        if tg.ndim != 2 or tg.shape[0] != B:
            raise ValueError(f"target_tokens: expected [{B},L], got {tuple(tg.shape)}")
        L = int(tg.shape[1])
        steps = max(L - 1, 0)
        shapes = (((B, steps), "i"), ((B, steps, V), "f"), ((B, steps), "f"), ((B,), "f"), ((B,), "i"), ((B,), "i"), ((B,), "i"))
        if on_dev:
            torch.cuda.current_stream(self.device).synchronize()
            bufs = [torch.empty(sh, dtype=torch.int32 if k == "i" else torch.float32, device=self.device) for sh, k in shapes]
            ptr = lambda a: ctypes.c_void_p(a.data_ptr())
            fn, what = self._lib.rv_teacher_forced_dev, "rv_teacher_forced_dev"
        else:
            bufs = [np.empty(sh, np.int32 if k == "i" else np.float32) for sh, k in shapes]
            ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
            fn, what = self._lib.rv_teacher_forced, "rv_teacher_forced"
        st = _capi.CRvScore(*[ptr(a) for a in bufs[2:]])
        if moves:
            if on_dev:
                mk = lambda dt: torch.empty((B, steps), dtype=dt, device=self.device)
                mv = Moves(*[mk(torch.int32 if k == 4 else torch.float32) for k in range(6)])
            else:
                mv = Moves(*[np.empty((B, steps), np.int32 if k == 4 else np.float32) for k in range(6)])
            sm = self._moves_struct(mv)
            fn = self._lib.rv_teacher_forced_moves_dev if on_dev else self._lib.rv_teacher_forced_moves
            self._check(fn(self._h, pr, pe, B, Tr, Te, L, ptr(tg), self._omit_mask(omit), ptr(bufs[0]), ptr(bufs[1]), ctypes.byref(st),
                           ctypes.byref(sm)), what.replace("forced", "forced_moves"))
            self.last_steps = steps
            as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(a)
            return ForcedScores(*[as_t(a) for a in bufs]), Moves(*[as_t(a) for a in mv])
        self._check(fn(self._h, pr, pe, B, Tr, Te, L, ptr(tg), self._omit_mask(omit), ptr(bufs[0]), ptr(bufs[1]), ctypes.byref(st)), what)
        self.last_steps = steps
        return ForcedScores(*[a if isinstance(a, torch.Tensor) else torch.from_numpy(a) for a in bufs])

    def align(self, input_data, target_tokens):
        """Forced alignment of known sequences: the forced decode of `teacher_forced_prediction` / `sequence_nll` with the moves of
        its steps kept (rv_teacher_forced_moves / _dev) -> (ForcedScores, Moves).  Moves: six [B,L-1] tensors; column t is the step
        that was fed target_tokens[b, t] and scored target_tokens[b, t+1], so it belongs to that label (as nll[b, t] does); -1 / 0
        where the label is the padding token.  `label_positions` cuts a row to its letters.  Host or device tensors follow the
        inputs; the ForcedScores is byte for byte that of the calls without moves."""
        return self._teacher_forced(input_data, target_tokens, self._train_omit, moves=True)

    def teacher_forced_prediction(self, input_data, target_tokens):
        """Decoder.call as _train_step uses it (basecaller.py:142-152, :234-244): the decoder is fed target_tokens[:, :-1] instead of
        its own argmax -> (sample_id [B,L-1] int32, rnn_output logits [B,L-1,V] f32), all L - 1 positions of every chunk."""
        r = self._teacher_forced(input_data, target_tokens, self._train_omit)
        return r.sample_id, r.logits

    def sequence_nll(self, input_data, target_tokens):
        """-> (nll [B,L-1] f32, nll_sum [B] f32): the cross-entropy of target_tokens[:, 1:] under the forced decode, 0 at the padding
        token; -nll_sum is each label row's log-likelihood given its chunk."""
        r = self._teacher_forced(input_data, target_tokens, self._train_omit)
        return r.nll, r.nll_sum

    def score_logits(self, real, pred, omit):
        """rv_score_logits: labels `real` [B,S] against logits `pred` [B,S,V] -> ForcedScores (sample_id = argmax of pred)."""
        t = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        lg = np.ascontiguousarray(t(pred), dtype=np.float32)
        lb = np.ascontiguousarray(t(real), dtype=np.int32)
        if lg.ndim != 3 or lg.shape[2] != self.cfg.vocab or lb.shape != lg.shape[:2]:
            raise ValueError(f"expected labels [B,S] and logits [B,S,{self.cfg.vocab}], got {lb.shape} and {lg.shape}")
        B, S = lb.shape
        ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
        pred_ids = np.empty((B, S), np.int32)
        outs = [np.empty((B, S), np.float32), np.empty(B, np.float32), np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32)]
        st = _capi.CRvScore(*[ptr(a) for a in outs])
        self._check(self._lib.rv_score_logits(self._h, ptr(lg), ptr(lb), B, S, self._omit_mask(omit), ptr(pred_ids), ctypes.byref(st)),
                    "rv_score_logits")
        return ForcedScores(*[torch.from_numpy(a) for a in [pred_ids, lg] + outs])

    def loss_function(self, real, pred):
        """basecaller.py:212-220: masked sparse cross-entropy of logits `pred` [B,S,V] at labels `real` [B,S] -> 0-d float32 tensor."""
        return self._quotients(self.score_logits(real, pred, ()))["loss"]

    def evaluate_step(self, data):
        """The forward half of _train_step (basecaller.py:225-253), no gradient: data = (raw, events, target) -> {'loss', 'acc'}
        of the forced decode, accuracy over the labels that are not padding, start or end token."""
        from .utils import unpack_data_to_input_target
        input_data, target_tokens = unpack_data_to_input_target(data, self.input_data_type)
        return self._quotients(self._teacher_forced(input_data, target_tokens, self._train_omit))

    def test_step(self, data):
        """_val_step (basecaller.py:264-279), what Keras evaluate() calls: greedy search, its logits and ids padded with zeros to
        L - 1 columns (tf.pad), then loss_function and masked_accuracy with [start, end] omitted -> {'loss', 'acc'}."""
        from .utils import unpack_data_to_input_target
        input_data, target_tokens = unpack_data_to_input_target(data, self.input_data_type)
        tg = target_tokens.detach().cpu().numpy() if isinstance(target_tokens, torch.Tensor) else np.asarray(target_tokens)
        L = int(tg.shape[1])
        tok, lg = self.greedy_search_prediction(input_data, L)
        B, S = tok.shape
        logits = np.zeros((B, max(L - 1, 0), self.cfg.vocab), np.float32)
        logits[:, :S] = lg.cpu().numpy()
        # masked_accuracy compares the padded ids; the library's pred is the argmax of the padded logits, which is the same thing: the greedy
        # ids are the argmax of their logits and a row of zero logits has its first maximum at id 0, tf.pad's fill
        return self._quotients(self.score_logits(tg[:, 1:], logits, self._val_omit))

    def _out_buffers(self, kind, B, steps, V):
        """Device outputs of the `*_dev` entry points.  Default: FRESH tensors per call, like the reference's return
        values (callers may keep one result per slab in a list); torch's caching allocator makes that cheap.
        `reuse_output_buffers = True` (explicit opt-in, bench.py's timed loop) returns views into one buffer per shape,
        valid only until the next call with that shape."""
        shape2 = (B, steps, V) if kind == "greedy" else (B, steps)
        if not getattr(self, "reuse_output_buffers", False):
            return (torch.empty((B, steps), dtype=torch.int32, device=self.device),
                    torch.empty(shape2, dtype=torch.float32, device=self.device))
        key = (kind, B, steps, V)
        cache = self.__dict__.setdefault("_outs", {})
        if key not in cache:
            cache.clear()
            cache[key] = (torch.empty((B, steps), dtype=torch.int32, device=self.device),
                          torch.empty(shape2, dtype=torch.float32, device=self.device))
        return cache[key]

    def beam_search_calls(self, input_data, beam_width, max_output_len, arrays: bool = False):
        """beam_search_prediction + the evaluators' post-processing fused on the device
        (ravvent_performance_evaluator.py:55,66-70): returns (seqs: list[str], probs: list[np.ndarray])
        where probs[i] = calc_prob_logits_beam_search_scores(scores)[i][:len(seqs[i])]."""
        keep, pr, pe, B, Tr, Te, on_dev = self._gather_inputs(input_data)
        if on_dev:   # host-buffer entry point: bring device tensors down (inputs are ~2 KB per chunk)
            return self.beam_search_calls(tuple(None if k is None else k.cpu().numpy() for k in keep)
                                          if self.input_data_type == "joint" else
                                          (keep[0] if keep[0] is not None else keep[1]).cpu().numpy(),
                                          beam_width, max_output_len, arrays)
        L = _as_int(max_output_len)
        steps = max(L - 1, 0)
        lut = self._call_lut()
        bases = np.zeros((B, steps), np.uint8); lens = np.zeros(B, np.int32); probs = np.zeros((B, steps), np.float32)
        S = ctypes.c_int32(0)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rv_beam_search_calls(self._h, pr, pe, B, Tr, Te, int(beam_width), L, p(lut), p(bases),
                                                   p(lens), p(probs), ctypes.byref(S)), "rv_beam_search_calls")
        self.last_steps = S.value
        if arrays:
            return bases, probs, lens
        flat = bases.tobytes()
        seqs = [flat[i * steps:i * steps + int(n)].decode("ascii") for i, n in enumerate(lens)]
        return seqs, [probs[i, :int(n)] for i, n in enumerate(lens)]

    def beam_search_call_arrays(self, input_data, beam_width, max_output_len):
        """beam_search_calls without per-chunk Python objects: (bases u8 [B, L-1], probs f32 [B, L-1], lengths i32 [B]),
        the layout `merger.Merger.merge_arrays` / `StreamingMerger.append` (rv_merge_calls) take."""
        return self.beam_search_calls(input_data, beam_width, max_output_len, arrays=True)

    def tokens_to_nuc_sequences(self, result_tokens):
        """basecaller.py:289-294.  [B,S,W] tokens (BeamHypotheses.tokens): a list of W strings per chunk."""
        if isinstance(result_tokens, torch.Tensor):
            result_tokens = result_tokens.detach().cpu().numpy()
        result_tokens = np.asarray(result_tokens)
        if result_tokens.ndim == 3:
            Bn, Sn, Wn = result_tokens.shape
            flat = self.tokens_to_nuc_sequences(np.ascontiguousarray(result_tokens.transpose(0, 2, 1)).reshape(Bn * Wn, Sn)) if Bn * Wn else []
            return [flat[b * Wn:(b + 1) * Wn] for b in range(Bn)]
        if self.tokenizer.word_index == nuc_tk.word_index:
            return tokens_to_strings(result_tokens)
        table = np.zeros(256, np.uint8)
        table[:8] = self._call_lut()                 # a custom tokenizer: its own letters, its own '' ^ $ dropped
        return tokens_to_strings(result_tokens, table)

    # ------------------------------------------------------------------ debug taps / profile
    def get_tensor(self, name: str) -> np.ndarray:
        n = ctypes.c_size_t(0)
        self._lib.rv_get_tensor(self._h, name.encode(), None, 0, ctypes.byref(n))
        out = np.empty(n.value, np.float32)
        self._check(self._lib.rv_get_tensor(self._h, name.encode(), out.ctypes.data_as(ctypes.c_void_p),
                                            out.size, ctypes.byref(n)), f"rv_get_tensor({name})")
        return out

    def profile(self) -> dict:
        buf = ctypes.create_string_buffer(4096)
        self._check(self._lib.rv_profile_names(self._h, buf, len(buf)), "rv_profile_names")
        out = {}
        for name in filter(None, buf.value.decode().split(";")):
            ms, n = ctypes.c_double(0), ctypes.c_int64(0)
            self._check(self._lib.rv_get_profile(self._h, name.encode(), ctypes.byref(ms), ctypes.byref(n)),
                        "rv_get_profile")
            out[name] = (ms.value, n.value)
        return out

    def reset_profile(self):
        self._check(self._lib.rv_reset_profile(self._h), "rv_reset_profile")
