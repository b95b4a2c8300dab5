"""The cases of tests/test_gru_gpu.py, shared with tests/test_gru.py, which proves on the numpy reference alone (tests/gru_reference.py)
that each one is a fair probe: the fp32 twin leaves the fp64 decode on at most B // 4 chunks, and no chunk is padding from end to end
unless the case says so.  A case is sized to where the BiGRU kernels can go wrong (the docstring of test_gru_gpu.py says what each
group probes); weights are the package's own init_weights for rnn 'bigru' under WEIGHTS_SEED with both bias rows of every cell drawn
non-zero (weights()), slabs synthetic.make_slab.

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

# the slab of the outer-interface tests (all beams, scoring, asynchronous calls, windows' shape, moves): two encoder layers, beam 5
CASES += [_c("world-beam5", 17, enc_depth=2, W=5, pads=(15, 3))]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
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
