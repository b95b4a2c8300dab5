"""The cases of tests/test_gru_gpu.py, shared with tests/test_gru.py, which proves on the numpy reference alone (tests/gru_reference.py)
that each one is a fair probe: the fp32 twin leaves the fp64 decode on at most B // 4 chunks, and no chunk is padding from end to end
unless the case says so.  A case is sized to where the BiGRU kernels can go wrong (the docstring of test_gru_gpu.py says what each
group probes); weights are the package's own init_weights for rnn 'bigru' under WEIGHTS_SEED with both bias rows of every cell drawn
non-zero (weights()), slabs synthetic.make_slab.  Beside the short cases (rows, tails, chaining, cell rows, searches, an all-padding chunk):
  lds-event-*   the layer-0 event form's LDS at 65,472 B (T_e = 115), 65,792 B (116, past 64 KB) and 141,312 B (352);
  long-*        352 raw samples, the chunker's 200 + 30, 100 + 252 (T_e > T_r, T_m = 352), Bahdanau at T_m = 352;
  gemm-k5       65 x (200 + 30): the three-block input GEMM with k = 5, as the shipped 1024 x 200 shape runs it (gemm_k asserts it);
and, apart from the case list, the adversarial weights of the encoder cells and of the decoder cells (at the end of this file).

fp64(rv, name) and twin_errors(rv, name) run the reference once per case and process: every test of a case shares the results and
leaves them as they are (the arrays are read-only)."""
import functools
from collections import namedtuple

import numpy as np

import gru_reference as G

WEIGHTS_SEED = 22
BIAS_SEED, BIAS_SCALE = 8, 0.3       # every cell's bias rows ~ N(0, 0.3^2): the size of a trained GRU's, far above every tolerance here
                                     # (seed 8: the first of 1..8 under which no case's decode stops at its first step; proven in test_gru.py)

Case = namedtuple("Case", "name B mode Tr Te enc_depth dec_depth attention W L slab_seed pads all_pad")
# W = 0: greedy search.  pads: (max_raw_pad, max_event_pad) of make_slab, None = its defaults.  all_pad: a chunk made padding from end to end.


def _c(name, B, mode="joint", Tr=50, Te=7, enc_depth=1, dec_depth=1, attention="luong", W=0, L=12, slab_seed=3, pads=None, all_pad=None):
    return Case(name, B, mode, Tr, Te, enc_depth, dec_depth, attention, W, L, slab_seed, pads, all_pad)


CASES = []
# recurrence rows: a lone chunk, a full workgroup, one live row beside fifteen clamped ones
# (seven events with make_slab's default of up to ten padded ones would leave four chunks in eleven all padding: at most three here)
# (slab seed 4: under seed 3 the lone event chunk emits the end token at its first step)
CASES += [_c(f"rows-B{B}-{mode}", B, mode, pads=(15, 3), slab_seed=4) for B in (1, 16, 17) for mode in ("raw", "event")]
# step-loop tails (T % 3) and direction edges (T = 1, 2), without trailing padding
CASES += [_c(f"tail-T{T}", 3, "joint", T, T, enc_depth=2, slab_seed=4, pads=(0, 0)) for T in (1, 2, 3, 4, 5)]
# state chaining and the 768-column GEMM: M = 119 rows (a partial 32-row tile), M = 300 and 60
CASES += [_c(f"chain-d{d}-B17", 17, "joint", 7, 7, enc_depth=d, slab_seed=5, pads=(2, 2)) for d in (2, 3)]
CASES += [_c(f"chain-d{d}-B5", 5, "joint", 60, 12, enc_depth=d, slab_seed=5) for d in (2, 3)]
CASES += [_c(f"chain-d2-{mode}", 17, mode, 7, 7, enc_depth=2, slab_seed=6, pads=(2, 2)) for mode in ("raw", "event")]
# decoder cell rows against the 64-row workgroup: N = B W = 1, 64, 65
# (slab seed 13: the first one under which the lone chunk of N = 1 decodes for more than a step or two with every cell stack)
CASES += [_c(f"cell-N{B * W}-dec{dd}-{att}", B, W=W, dec_depth=dd, attention=att, slab_seed=13)
          for B, W in ((1, 1), (8, 8), (13, 5)) for dd, att in ((1, "luong"), (2, "luong"), (3, "luong"), (1, "bahdanau"))]
CASES += [_c(f"search-{'greedy' if W == 0 else 'beam%d' % W}-{att}", 17, W=W, attention=att)
          for W, att in ((0, "luong"), (1, "luong"), (2, "luong"), (5, "luong"), (8, "luong"), (0, "bahdanau"), (5, "bahdanau"))]
# one all-padding chunk in a slab
CASES += [_c(f"allpad-{'greedy' if W == 0 else 'beam%d' % W}", 5, W=W, enc_depth=2, slab_seed=4, all_pad=2) for W in (0, 3)]

# LDS edges of the layer-0 event form, gru_lds_bytes(5, T) = 28,672 + 320 T: T = 115 the last window under 64 KB, 116 the first one that
# needs the opt-in of configure_gru_kernels, 352 the decode's limit (141,312 B); up to ten padded events, none of 115 all padding
CASES += [_c(f"lds-event-T{T}", 17, "event", Te=T, enc_depth=d, W=3, L=6, slab_seed=4, pads=(0, 10)) for T, d in ((115, 2), (116, 2), (352, 1))]
# long windows: the F = 1 form and the F = 0 ring over 352 steps; the chunker's own 200 + 30 (raw M = 3,400: k = 2 of the three-block
# GEMM); 100 + 252, T_e > T_r, T_m = 352 through the per-step attend
CASES += [_c("long-raw-T352", 17, "raw", Tr=352, enc_depth=2, L=6, slab_seed=4)]
CASES += [_c(f"long-joint-{Tr}+{Te}", 17, "joint", Tr, Te, enc_depth=2, W=5, L=8, slab_seed=4) for Tr, Te in ((200, 30), (100, 252))]
# the two-pass Bahdanau attend at the memory limit under a GRU cell, N = 40
CASES += [_c("long-bahdanau-T352", 5, "event", Te=352, attention="bahdanau", W=8, L=6, slab_seed=4)]
# the three-block GEMM as the shipped shape (1024 chunks x 200 samples) runs it: raw M = 13,000, ntile = 407 > 384, k = 5; event M = 1,950, k = 1
CASES += [_c("gemm-k5", 65, "joint", 200, 30, enc_depth=2, W=1, L=4, slab_seed=4)]

# the slab of the outer-interface tests (all beams, scoring, asynchronous calls, windows' shape, moves): two encoder layers, beam 5
CASES += [_c("world-beam5", 17, enc_depth=2, W=5, pads=(15, 3))]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def gemm_k(c):
    """{encoder: row-group multiple k of the three-block input GEMM of its layers >= 1}, from the launcher's arithmetic as
    tests/test_gemm_probe_gpu.py restates it (M = B T rows)."""
    from test_gemm_probe_gpu import ws_geometry
    T = {"raw": c.Tr if c.mode != "event" else 0, "event": c.Te if c.mode != "raw" else 0}
    return {e: ws_geometry(c.B * t, ncb=3)[0] for e, t in T.items() if t and c.enc_depth > 1}


# the cases named for a GEMM geometry reach it: a change of the launcher must not make them stop doing so unnoticed
assert gemm_k(BY_NAME["gemm-k5"]) == {"raw": 5, "event": 1}
assert gemm_k(BY_NAME["long-joint-200+30"])["raw"] == 2
assert all(set(gemm_k(c).values()) <= {1} for c in CASES if not c.name.startswith(("long-", "gemm-", "lds-")))   # ... and no earlier case did
WORLD = BY_NAME["world-beam5"]


def config(rv, c, **kw):
    return rv.config.RvConfig(enc_depth=c.enc_depth, dec_depth=c.dec_depth, mode=c.mode, attention=c.attention, rnn="bigru",
                              max_batch=kw.get("max_batch", max(c.B, 1)), max_raw_len=max(c.Tr, 1), max_event_len=max(c.Te, 1),
                              max_output_len=max(c.L, 2), max_beam=max(c.W, 1))


def slab(rv, c):
    kw = {} if c.pads is None else dict(max_raw_pad=c.pads[0], max_event_pad=c.pads[1])
    raw, ev, _ = rv.synthetic.make_slab(c.B, c.Tr, c.Te, seed=c.slab_seed, **kw)
    if c.all_pad is not None:
        raw[c.all_pad] = 0.0
        ev[c.all_pad] = 0.0
    return raw, ev


@functools.lru_cache(maxsize=None)
def weights(rv, enc_depth, dec_depth, mode, attention):
    cfg = rv.config.RvConfig(enc_depth=enc_depth, dec_depth=dec_depth, mode=mode, attention=attention, rnn="bigru")
    flat = rv.weights.init_weights(cfg, seed=WEIGHTS_SEED)
    # init_weights leaves a GRU's biases at zero; a trained model's are not.  Both rows of every cell's bias -- b[0] beside x.W, b[1]
    # beside h.U and, for the candidate gate, inside the reset product -- are drawn non-zero here, so that a dropped term, swapped rows
    # or b[1]_h added outside r * (.) shows in every case
    rng = np.random.default_rng(BIAS_SEED)
    for name in sorted(flat):
        if name.endswith(".b"):
            flat[name] = (BIAS_SCALE * rng.standard_normal(flat[name].shape)).astype(np.float32)
    return flat, rv.weights.flat_to_nested(cfg, flat)


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    return x


def keep_rows(c):
    """The chunks whose tensors are compared as numbers (every chunk but an all-padding one, whose logits and alignments are NaN)."""
    return [b for b in range(c.B) if b != c.all_pad]


def sliced(out, taps, keep):
    """The reference's results and taps on the chunks `keep` alone (chunks never interact: the values are those of a slab of them)."""
    rows0 = ("enc_output", "mask", "keys", "lengths", "finished", "log_probs")
    t = {k: (v if v is None else (v[keep] if k in rows0 else v[:, keep])) for k, v in taps.items()}
    return tuple(a[keep] for a in out), t


@functools.lru_cache(maxsize=None)
def fp64(rv, name):
    """-> dict(raw, ev, w, cfg, out = (tokens, scores) or (ids, logits), taps) of the case in fp64, read-only."""
    c = BY_NAME[name]
    raw, ev = slab(rv, c)
    _, w = weights(rv, c.enc_depth, c.dec_depth, c.mode, c.attention)
    cfg = config(rv, c).oracle_cfg()
    taps = {}
    if c.W == 0:
        out = G.greedy_search(w, cfg, raw, ev, c.L, taps=taps)
    else:
        out = G.beam_search(w, cfg, raw, ev, c.W, c.L, taps=taps)
    return _freeze(dict(raw=raw, ev=ev, w=w, cfg=cfg, out=tuple(_freeze(a) for a in out), taps=taps))


@functools.lru_cache(maxsize=None)
def twin_errors(rv, name):
    """{tensor: max |fp32 twin - fp64|} of the case over its compared chunks (test_parity_gpu._twin_greedy / _twin_beam, which also hold
    the twin to the fp64 decode on all but B // 4 chunks: _stays)."""
    from test_parity_gpu import _twin_beam, _twin_greedy
    c, r = BY_NAME[name], fp64(rv, name)
    keep = keep_rows(c)
    out, taps = sliced(r["out"], r["taps"], keep)
    raw, ev = r["raw"][keep], r["ev"][keep]
    if c.W == 0:
        return _twin_greedy(G, r["w"], r["cfg"], raw, ev, c.L, out[0], out[1], taps, name)
    return _twin_beam(G, r["w"], r["cfg"], raw, ev, c.W, c.L, taps, out[1], name)


# ---------------------------------------------------------------------------------------------- adversarial weights
# k_gru_rec_mx holds U^T as split-f16 fragments with one power-of-two factor per gate column and h as a 2^14-scaled f16 pair that rests
# on |h| <= 1; k_dec_cell_gru multiplies in f32.  The recipes are those of the BiLSTM tests (test_bench_config_gpu, test_config5_gpu)
# on the GRU's gate order z, r, h: one recurrent row x 30 (every column's largest element then sits in that row and the others lose five
# bits of the first part's range), one row x 1e-5 (deep in the second part / the f16 subnormals of its columns), gained gate columns
# (factors apart from their neighbours'; pre-activations of tens, whose activation error the gain multiplies step after step).
ADV_B, ADV_TR, ADV_TE = 17, 150, 25
ADV_GAINS = (8.0, 50.0)
ADV_COLS = (5, 300, 296)             # one z column, two h columns of every encoder cell's U
ADV_DEC = dict(B=6, Tr=60, Te=12, W=5, L=16, slab_seed=3, cols=(256 + 5, 256 + 77))


def _adversarial_encoder_flat(rv, col_gain, saturate):
    flat, _ = weights(rv, 2, 1, "joint", "luong")
    flat = {k: v.copy() for k, v in flat.items()}
    for name in sorted(flat):
        if name.startswith("enc_") and name.endswith(".U"):
            U = flat[name]
            U[17, :] *= 30.0
            U[90, :] *= 1e-5
            for col in ADV_COLS:
                U[:, col] *= col_gain
        if saturate and name.startswith("enc_") and name.endswith(".b"):
            b = flat[name]
            b[0, 0:64] = -20.0                                        # z closed: h' = the candidate
            b[0, 256:320] = 20.0 * (1 - 2 * (np.arange(64) % 2))      # ... which sits at +1 and -1 in turn
    return flat


@functools.lru_cache(maxsize=None)
def adversarial_encoder(rv, col_gain, saturate):
    """-> dict(flat, raw, ev, enc_output, keys, mask (fp64), twin {enc_output, keys: max |fp32 twin - fp64|}, saturated (the share of
    |enc_output| within 2^-20 of 1), preact (the largest |h . U + b[1]| of a gained column over the last layer's steps)), read-only."""
    from oracle.ravvent_oracle import setup_memory
    flat = _adversarial_encoder_flat(rv, col_gain, saturate)
    cfg = rv.config.RvConfig(enc_depth=2, dec_depth=1, mode="joint", attention="luong", rnn="bigru")
    w = rv.weights.flat_to_nested(cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(ADV_B, ADV_TR, ADV_TE, seed=3)
    res = {}
    for dt in (np.float64, np.float32):
        enc, mask = G.encode_input(w, raw, ev, "joint", 0.0, dt)
        keys, _ = setup_memory(w, enc, mask, dt)
        res[dt] = (enc, keys, mask)
    enc, keys, mask = res[np.float64]
    twin = dict(enc_output=float(np.abs(res[np.float32][0] - enc).max()), keys=float(np.abs(res[np.float32][1] - keys).max()))
    pre = 0.0
    for e, seg in (("enc_raw", slice(0, ADV_TR)), ("enc_event", slice(ADV_TR, ADV_TR + ADV_TE))):
        for d, half in (("fwd", slice(0, 128)), ("bwd", slice(128, 256))):
            _, U, b = (np.asarray(a, np.float64) for a in w[e][1][d])
            hr = enc[:, seg, half] @ U[:, list(ADV_COLS)] + b[1, list(ADV_COLS)]      # what the step after each output step adds to the gate
            pre = max(pre, float(np.abs(hr).max()))
    saturated = float((np.abs(np.abs(enc) - 1.0) <= 2.0 ** -20).mean())
    return _freeze(dict(flat=flat, raw=raw, ev=ev, enc_output=enc, keys=keys, mask=mask, twin=twin, saturated=saturated, preact=pre))


@functools.lru_cache(maxsize=None)
def adversarial_decoder(rv, dec_depth):
    """The decoder cells' recurrent kernels under stress: two h-gate columns x 50, one row x 30, one row x 1e-5, the end token suppressed so
    that every chunk runs all L - 1 steps.  -> dict(flat, raw, ev, w, cfg, out, taps) in fp64 as fp64() gives them, and twin = the fp32
    twin's errors (test_parity_gpu._twin_beam, which holds the twin to the fp64 decode on all but B // 4 chunks)."""
    from test_parity_gpu import _twin_beam
    a = ADV_DEC
    c = _c(f"adversarial-dec{dec_depth}", a["B"], "joint", a["Tr"], a["Te"], dec_depth=dec_depth, W=a["W"], L=a["L"], slab_seed=a["slab_seed"])
    flat, _ = weights(rv, 1, dec_depth, "joint", "luong")
    flat = {k: v.copy() for k, v in flat.items()}
    for k in range(dec_depth):
        U = flat[f"dec_cells.{k}.U"]
        for col in a["cols"]:
            U[:, col] *= 50.0
        U[3, :] *= 30.0
        U[90, :] *= 1e-5
    rcfg = config(rv, c)
    flat["b_fc"][rcfg.end_token] = -30.0
    w = rv.weights.flat_to_nested(rcfg, flat)
    raw, ev = slab(rv, c)
    cfg = rcfg.oracle_cfg()
    taps = {}
    out = G.beam_search(w, cfg, raw, ev, c.W, c.L, taps=taps)
    twin = _twin_beam(G, w, cfg, raw, ev, c.W, c.L, taps, out[1], c.name)
    return _freeze(dict(case=c, flat=flat, raw=raw, ev=ev, w=w, cfg=cfg, out=tuple(_freeze(x) for x in out), taps=taps, twin=twin))
