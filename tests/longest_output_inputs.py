"""The inputs of tests/test_longest_output_gpu.py and the conditions they must meet, on the oracle alone (no GPU, no library).

passes() runs oracle.beam_search once in fp64 and once as its numpy fp32 twin for one (family, inputs, W, shape) and derives, in fp64,
everything the whole-beam outputs are compared with: the scores of all W slots (a replay of the beam steps over the tapped logits),
the back-traced tokens and the path scores.  Both passes are cached: the CPU companion and every GPU test share one computation.
The assert_* functions state the conditions of the module docstring of test_longest_output_gpu on a set of records -- the oracle's
in the companion, the GPU's own in the GPU module."""
import numpy as np

from test_beams_gpu import _expect
from test_kernel_forms_gpu import _slab
from test_parity_gpu import _emitting_flat

L = 64
STEPS = L - 1
HALF = 32                                   # the second half of the lane = step wave, and of the 64-bit ballot
TWIN_SCORE_BOUND = 4e-5                     # 2 x this + 5e-6 (_assert_twin) stays below the project's 1e-4
# shape -> (T_r, T_e, chunks of _slab taken)
SHAPES = {"A": (40, 8, slice(None)), "C": (308, 44, [1, 2])}
# inputs -> (weight seed, end-token bias, slab seed) of _emitting_flat / _slab
INPUTS = {"long": (22, -1.0, 1), "spread": (22, 1.5, 1), "ragged": (24, 1.0, 1)}
# the B = 70 slab of the decode_split form (synthetic.make_slab): inputs -> (weight seed, end-token bias, slab seed)
SPLIT_B = 70
SPLIT_INPUTS = {"long": (22, -1.0, 8), "spread": (22, 1.5, 2)}
# family -> (attention, decoder cells, beam widths)
FAMILIES = {"luong1": ("luong", 1, (1, 5, 8)), "bahdanau1": ("bahdanau", 1, (1, 5, 8)), "luong2": ("luong", 2, (5,))}


def inputs_for(kind, W):
    """The inputs that serve a kind of case ("long" / "spread") at beam W: with one hypothesis per chunk the "spread" weights end five
    chunks at their first step, and the "ragged" ones spread the finishing steps instead."""
    return "ragged" if (kind, W) == ("spread", 1) else kind


# every (family, inputs, W, shape, split) the GPU module decodes
ALL = [(fam, inputs_for(kind, W), W, "A", False) for fam, (_, _, ws) in FAMILIES.items() for W in ws for kind in ("long", "spread")] + \
      [("luong1", kind, 5, "C", False) for kind in ("long", "spread")] + [("luong1", kind, 5, "A", True) for kind in ("long", "spread")]


def config(rv, fam, shape="A", max_batch=6):
    attention, D, _ = FAMILIES[fam]
    TR, TE, _ = SHAPES[shape]
    return rv.RvConfig(mode="joint", attention=attention, dec_depth=D, max_batch=max_batch, max_raw_len=TR, max_event_len=TE,
                       max_output_len=L, max_beam=8)


def flat_weights(rv, cfg, name, split=False):
    seed, bias, _ = (SPLIT_INPUTS if split else INPUTS)[name]
    return _emitting_flat(rv, cfg, seed=seed, end_bias=bias)


def slab(rv, name, shape="A", split=False):
    TR, TE, rows = SHAPES[shape]
    if split:
        raw, ev, _ = rv.synthetic.make_slab(SPLIT_B, TR, TE, seed=SPLIT_INPUTS[name][2])
    else:
        raw, ev = _slab("joint", TR, TE, seed=INPUTS[name][2])
        raw, ev = np.ascontiguousarray(raw[rows]), np.ascontiguousarray(ev[rows])
    for a in (raw, ev):
        a.setflags(write=False)
    return raw, ev


def _path(osc, opar, oln):
    """The scores [S,B,W] along each hypothesis's back-trace -> [B,S,W], repeated past the chunk's longest hypothesis."""
    S, nB, W = osc.shape
    path = np.zeros((nB, S, W), osc.dtype)
    for b in range(nB):
        Lb = min(S, int(oln[b].max()))
        for k in range(W):
            p = k
            for t in range(Lb - 1, -1, -1):
                path[b, t, k] = osc[t, b, p]
                p = opar[t, b, p]
            path[b, Lb:, k] = path[b, Lb - 1, k]
    return path


def _replay(oracle, lg, W, end):
    """The beam steps over step logits lg [S,B,W,V] in lg's own precision -> ids, parents, the scores of all W slots [S,B,W], lengths."""
    nB = lg.shape[1]
    lp = np.full((nB, W), -np.inf, lg.dtype); lp[:, 0] = 0.0
    fin, ln = np.zeros((nB, W), bool), np.zeros((nB, W), np.int64)
    ids, par, sc = [], [], []
    for s in range(lg.shape[0]):
        top, word, parent, lp, fin, ln = oracle.beam_search_step(lg[s], lp, fin, ln, end)
        ids.append(word); par.append(parent); sc.append(top)
    return np.stack(ids), np.stack(par), np.stack(sc), ln


def _one_pass(oracle, w, cfg, raw, ev, W, dtype):
    taps = {}
    tok, top1 = oracle.beam_search(w, cfg, raw, ev, W, L, dtype=dtype, taps=taps)
    end = cfg["end_token"]
    ids, par, sc, ln = _replay(oracle, taps["step_logits"], W, end)
    assert (ids == taps["step_ids"]).all() and (par == taps["parent_ids"]).all() and (ln == taps["lengths"]).all()
    tokens = np.transpose(oracle.gather_tree(taps["step_ids"], taps["parent_ids"], ln.max(1), end), (1, 0, 2))
    return dict(taps=taps, top1=top1, ids=ids, par=par, sc=sc, lengths=ln, tokens=tokens, scores=np.transpose(sc, (1, 0, 2)),
                path_scores=_path(sc, par, ln), log_probs=sc[-1])


def max_error(x, ref):
    """max |x - ref| over the finite entries of ref; where ref is infinite (the slots a first step cannot fill: W > V) x must equal it."""
    x, ref = np.asarray(x), np.asarray(ref)
    fin = np.isfinite(ref)
    assert x.shape == ref.shape and np.array_equal(x[~fin], ref[~fin]), "infinite entries differ"
    return float(np.abs(x[fin].astype(np.float64) - ref[fin]).max(initial=0.0))


_PASSES = {}


def passes(rv, oracle, fam, name, W, shape="A", split=False):
    """-> dict(o: the fp64 pass, t: the fp32 twin's, e: _expect of the fp64 records, w, cfg, raw, ev, twin: the twin's errors)."""
    key = (fam, name, W, shape, split)
    if key not in _PASSES:
        cfg = config(rv, fam, shape, SPLIT_B if split else 6)
        w = rv.weights.flat_to_nested(cfg, flat_weights(rv, cfg, name, split))
        raw, ev = slab(rv, name, shape, split)
        o = _one_pass(oracle, w, cfg.oracle_cfg(), raw, ev, W, np.float64)
        t = _one_pass(oracle, w, cfg.oracle_cfg(), raw, ev, W, np.float32)
        S, nB = o["ids"].shape[:2]
        e = _expect(oracle, o["ids"], o["par"], o["sc"], np.full(nB, S), cfg.end_token)
        twin = {}
        if t["ids"].shape == o["ids"].shape:
            twin = {k: max_error(t[k], o[k]) for k in ("scores", "path_scores", "log_probs")}
            twin["step_logits"] = float(np.abs(t["taps"]["step_logits"] - o["taps"]["step_logits"]).max())
        _PASSES[key] = dict(o=o, t=t, e=e, w=w, cfg=cfg, raw=raw, ev=ev, twin=twin)
    return _PASSES[key]


# ---------------------------------------------------------------------------------------------- the conditions on a set of records
def assert_twin_follows(p, tag):
    """The numpy fp32 twin returns the fp64 pass's ids and parents on every chunk for every step, and its scores are within
    TWIN_SCORE_BOUND: a condition on the inputs."""
    o, t = p["o"], p["t"]
    assert t["ids"].shape == o["ids"].shape, (tag, "the twin runs other steps", t["ids"].shape, o["ids"].shape)
    left = [b for b in range(o["ids"].shape[1]) if (t["ids"][:, b] != o["ids"][:, b]).any() or (t["par"][:, b] != o["par"][:, b]).any()]
    assert not left, (tag, "the twin leaves the fp64 decode on chunks", left)
    assert (t["lengths"] == o["lengths"]).all() and (t["tokens"] == o["tokens"]).all(), tag
    worst = max(p["twin"][k] for k in ("scores", "path_scores", "log_probs"))
    assert worst <= TWIN_SCORE_BOUND, (tag, "the twin's scores", p["twin"])


def assert_long(e, W, tag):
    """e: an _expect of records.  Every hypothesis of every chunk runs all 63 steps; beyond W = 1 a live parent at a step >= 56 is not
    the identity and a hypothesis w > 0 differs from hypothesis 0 in a column >= 32."""
    S = e["tokens"].shape[1]
    assert S == STEPS and (e["lengths"] == STEPS).all(), (tag, "a hypothesis ends early", S, e["lengths"].tolist())
    if W == 1:
        return
    ident = np.arange(W)[None, None]
    assert (e["par"][56:] != ident).any(), (tag, "every parent from step 56 is the identity")
    assert (e["par"][HALF:] != ident).sum() >= 8, (tag, "hardly a slot changes after step 32")
    tok = e["tokens"]
    assert (tok[:, HALF:, 1:] != tok[:, HALF:, :1]).any(), (tag, "every hypothesis equals hypothesis 0 from column 32")


def assert_spread(e, W, tag):
    """At least one chunk runs all 63 steps, at least one is finished before step 32, the finishing steps take three values or more
    (two on a slab of two chunks)."""
    fin = e["fin_at"]
    assert e["tokens"].shape[1] == STEPS and (fin == STEPS).any(), (tag, "no chunk runs all 63 steps", fin.tolist())
    assert (fin < HALF).any() and len(set(fin.tolist())) >= min(3, len(fin)), (tag, "finishing steps", fin.tolist())


def assert_ragged(tokens, tag):
    """tokens [B,S] of the best hypothesis: the letter counts take four values or more, one is 63, and one row has a
    non-letter id before its last letter."""
    letters = tokens >= 3
    counts = letters.sum(1)
    assert len(set(counts.tolist())) >= 4 and (counts == STEPS).any(), (tag, "letter counts", counts.tolist())
    inner = [b for b in range(tokens.shape[0]) if counts[b] and not letters[b, :np.nonzero(letters[b])[0][-1]].all()]
    assert inner, (tag, "no row has a non-letter id before its last letter")
    return counts, inner


_GREEDY = {}
GREEDY_EARLY_ROWS = (3, 4, 5)            # chunks of the "ragged" slab whose greedy search ends after a few steps


def greedy_passes(rv, oracle, rows=None):
    """oracle.greedy_search at L = 64 on the "ragged" weights (Luong, one cell), on all six chunks or on `rows` of them, in fp64 and as
    the numpy fp32 twin -> dict(og, olg, tg, tlg, gtaps, w, cfg, raw, ev)."""
    key = None if rows is None else tuple(rows)
    if key not in _GREEDY:
        cfg = config(rv, "luong1")
        w = rv.weights.flat_to_nested(cfg, flat_weights(rv, cfg, "ragged"))
        raw, ev = slab(rv, "ragged")
        if rows is not None:
            raw, ev = np.ascontiguousarray(raw[list(rows)]), np.ascontiguousarray(ev[list(rows)])
        gtaps = {}
        og, olg = oracle.greedy_search(w, cfg.oracle_cfg(), raw, ev, L, dtype=np.float64, taps=gtaps)
        tg, tlg = oracle.greedy_search(w, cfg.oracle_cfg(), raw, ev, L, dtype=np.float32)
        _GREEDY[key] = dict(og=og, olg=olg, tg=tg, tlg=tlg, gtaps=gtaps, w=w, cfg=cfg, raw=raw, ev=ev)
    return _GREEDY[key]
