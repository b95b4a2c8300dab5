"""A chunk that is padding from end to end inside a slab of ordinary chunks.

Every memory step of such a chunk is masked, so each attention kernel takes its all-masked branch: the softmax is 0 / 0 = NaN like
the reference's (the fp64 oracle masks scores with -inf), the logits and scores of the chunk are NaN, and the beam step ranks NaN
candidates (wave_max_fast + the ballot tie rule: the first free lane wins, so the chunk's tokens are all 0, as numpy's argsort /
argmax give them).  The chunk never emits the end token, so the slab runs all L - 1 steps.  These tests pin that behaviour against
the fp64 oracle -- tokens exact, scores within 1e-4 with NaN where the oracle has NaN, the same step count -- at the first, a middle
and the last position of the slab, in every input mode, for both attention types, one and two decoder cells, beams 1 / 5 / 8,
greedy search, the per-step kernels, and the call paths that run the slab as a whole (asynchronous calls, fused post-processing,
slab graph replay, sub-slabs).  And they show that the chunk's neighbours do not see it: their tokens and score bits equal those of
the same slab decoded without the padding chunk on the columns both have, and the oracle's end-token padding beyond."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4
B, TR, TE, L = 5, 60, 12, 18


def _slab(rv, mode, n, pos, seed=13):
    raw, ev, _ = rv.synthetic.make_slab(n, TR, TE, seed=seed)
    raw[pos] = 0.0
    ev[pos] = 0.0
    return raw, ev


def _x(mode, raw, ev):
    return {"joint": (raw, ev), "raw": raw, "event": ev}[mode]


def _mk(rv, mode, attention, dec_depth, max_batch=B):
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, decoder_depth=dec_depth, attention_type=attention,
                       honor_attention_type=True, max_batch=max_batch, max_raw_len=TR, max_event_len=TE, max_output_len=L)
    flat = rv.weights.init_weights(bc.cfg, seed=13)
    flat["b_fc"][bc.cfg.end_token] = 0.5            # ordinary chunks finish after a step or two
    bc.set_weights_flat(flat)
    return bc, rv.weights.flat_to_nested(bc.cfg, flat)


def _oracle(oracle, bc, w, mode, raw, ev, W):
    cfg = bc.cfg.oracle_cfg()
    r, e = (raw if mode != "event" else None), (ev if mode != "raw" else None)
    if W == "greedy":
        return oracle.greedy_search(w, cfg, r, e, L)
    return oracle.beam_search(w, cfg, r, e, W, L)


def _run(bc, mode, raw, ev, W):
    if W == "greedy":
        t, s = bc.greedy_search_prediction(_x(mode, raw, ev), L)
    else:
        t, s = bc.beam_search_prediction(_x(mode, raw, ev), W, L)
    return t.numpy().copy(), s.numpy().copy()


def _assert_oracle(tok, sc, otok, osc, pos, tag):
    """Tokens exact, scores (greedy: logits) within 1e-4, NaN exactly where the oracle's are; the padding chunk is NaN all through."""
    assert tok.shape == otok.shape, (tag, tok.shape, otok.shape)
    assert (tok == otok).all(), tag
    assert np.array_equal(np.isnan(sc), np.isnan(osc)), tag
    assert np.isnan(sc[pos]).all() and (tok[pos] == 0).all(), tag
    fin = ~np.isnan(osc)
    assert np.abs(sc[fin] - osc[fin]).max(initial=0.0) < TOL, tag


def _assert_neighbours(tok, sc, rtok, rsc, pos, end, tag):
    """Rows other than `pos` == the slab decoded without it (rtok / rsc): token and score bits on the common columns; beyond them the
    end-token padding (beam search) -- a greedy row keeps sampling after its own end token, so there the oracle check stands alone."""
    keep = [b for b in range(tok.shape[0]) if b != pos]
    S = rtok.shape[1]
    assert tok.shape[1] >= S, tag
    assert (tok[keep, :S] == rtok).all(), tag
    assert np.array_equal(sc[keep, :S].view(np.uint32), rsc.view(np.uint32)), tag
    if sc.ndim == 2:
        assert (tok[keep, S:] == end).all(), tag


CASES = [  # mode, attention, decoder depth, beam (or "greedy"), options
    ("joint", "luong", 1, 5, {}), ("raw", "luong", 1, 5, {}), ("event", "luong", 1, 5, {}),
    ("joint", "bahdanau", 1, 5, {}), ("joint", "luong", 2, 5, {}), ("joint", "bahdanau", 1, 1, {}),
    ("joint", "luong", 1, 1, {}), ("joint", "luong", 1, 8, {}), ("joint", "luong", 1, "greedy", {}),
    ("joint", "luong", 2, "greedy", {}), ("joint", "bahdanau", 1, "greedy", {}),
    ("joint", "luong", 1, 5, {"matrix_attention": 0}), ("joint", "luong", 1, 5, {"matrix_attention": 1, "matrix_cell": 0}),
    ("joint", "bahdanau", 1, 5, {"matrix_cell": 0}), ("joint", "luong", 2, 5, {"matrix_cell": 0}),
    ("joint", "luong", 1, 5, {"persistent_decode": 0}), ("joint", "luong", 1, 5, {"persistent_decode": 0, "flash_attend": 0}),
    ("joint", "bahdanau", 1, 5, {"persistent_decode": 0}), ("joint", "luong", 1, "greedy", {"persistent_decode": 0}),
]


@pytest.mark.parametrize("pos", [0, B // 2, B - 1], ids=["first", "middle", "last"])
@pytest.mark.parametrize("mode,attention,dec_depth,W,opts", CASES,
                         ids=[f"{m}-{a}-d{d}-{w}" + "".join(f"-{k}{v}" for k, v in o.items()) for m, a, d, w, o in CASES])
def test_all_padding_chunk_matches_oracle_and_spares_neighbours(rv, oracle, mode, attention, dec_depth, W, opts, pos):
    bc, w = _mk(rv, mode, attention, dec_depth)
    for k, v in opts.items():
        bc.set_option(k, v)
    raw, ev = _slab(rv, mode, B, pos)
    tok, sc = _run(bc, mode, raw, ev, W)
    otok, osc = _oracle(oracle, bc, w, mode, raw, ev, W)
    assert otok.shape[1] == L - 1                        # the padding chunk never finishes: the slab runs every step
    _assert_oracle(tok, sc, otok, osc, pos, (mode, attention, dec_depth, W, opts, pos))
    keep = [b for b in range(B) if b != pos]
    rtok, rsc = _run(bc, mode, raw[keep], ev[keep], W)
    _assert_neighbours(tok, sc, rtok, rsc, pos, bc.cfg.end_token, (mode, attention, dec_depth, W, opts, pos))
    bc.close()


def test_all_padding_chunk_on_the_slab_wide_call_paths(rv, oracle):
    """The call paths that handle the slab as a whole, on one slab with a padding chunk in the middle: asynchronous submit / collect
    (depth 2, byte-identical to the synchronous call), the fused post-processing (the padding chunk calls no base; the other rows'
    calls equal the host form of the synchronous tokens and scores), slab_graph replay (byte-identical, twice), and a slab of 70
    chunks decoded by the per-step kernels as two concurrent sub-slabs (decode_split 2) with the padding chunk in the first: the other sub-slab is extended
    by k_dec_finalize to the slab's L - 1 steps, and every row equals the oracle and the slab without the padding chunk."""
    import torch
    W, pos = 5, 2
    bc, w = _mk(rv, "joint", "luong", 1, max_batch=70)
    raw, ev = _slab(rv, "joint", B, pos)
    tok, sc = _run(bc, "joint", raw, ev, W)
    otok, osc = _oracle(oracle, bc, w, "joint", raw, ev, W)
    _assert_oracle(tok, sc, otok, osc, pos, "sync")

    dev = (torch.from_numpy(raw).cuda(), torch.from_numpy(ev).cuda())
    bc.set_async_depth(2)
    for t, s in bc.beam_search_stream([dev, (raw, ev), dev], W, L):
        assert (t.cpu().numpy() == tok).all() and np.array_equal(s.cpu().numpy().view(np.uint32), sc.view(np.uint32)), "async"

    bases, probs, lens = bc.beam_search_call_arrays((raw, ev), W, L)
    seqs = bc.tokens_to_nuc_sequences(torch.from_numpy(tok))
    with np.errstate(invalid="ignore"):
        pref = rv.utils.calc_prob_logits_beam_search_scores(torch.from_numpy(sc)).numpy()
    assert lens[pos] == 0 and seqs[pos] == ""
    for b in range(B):
        assert bases[b, :lens[b]].tobytes().decode("ascii") == seqs[b], b
        assert np.abs(probs[b, :lens[b]] - pref[b, :lens[b]]).max(initial=0.0) < 1e-6, b
    for k, (sq, pr) in enumerate(zip(*bc.beam_search_calls((raw, ev), W, L))):
        assert sq == seqs[k]

    bc.set_option("slab_graph", 1)
    for _ in range(2):
        t, s = _run(bc, "joint", raw, ev, W)
        assert (t == tok).all() and np.array_equal(s.view(np.uint32), sc.view(np.uint32)), "slab_graph"
    bc.set_option("slab_graph", 0)

    Bw, posw = 70, 10                                      # sub-slabs: chunks 0-34 | 35-69
    raw, ev = _slab(rv, "joint", Bw, posw, seed=14)
    bc.set_option("persistent_decode", 0)                 # (the persistent decode is one launch for the whole slab)
    bc.set_option("decode_split", 2)
    tok, sc = _run(bc, "joint", raw, ev, W)
    otok, osc = _oracle(oracle, bc, w, "joint", raw, ev, W)
    _assert_oracle(tok, sc, otok, osc, posw, "decode_split 2")
    keep = [b for b in range(Bw) if b != posw]
    rtok, rsc = _run(bc, "joint", raw[keep], ev[keep], W)
    _assert_neighbours(tok, sc, rtok, rsc, posw, bc.cfg.end_token, "decode_split 2")
    bc.close()
