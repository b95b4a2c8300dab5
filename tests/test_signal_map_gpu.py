"""The signal map on the GPU: calls with positions (rv_beam_search_*calls_moves), forced alignment
(rv_teacher_forced_moves*), and Basecaller.basecall(..., moves=True).

Shapes: B = 5 chunks, joint 50 + 7 (raw 57 / event 33 once each), L = 12; chunk 3 is padded from its middle on, chunk 4 is padding from
end to end.  Weights are test_parity_gpu._emitting_flat's, so that the calls are strings.  Every comparison with an existing call is
bit for bit; the forced moves are held to the fp64 statement of tests/signal_map_reference.py with the tolerances of
test_moves_gpu.test_against_fp64 (alignments within 1e-4; with d the measured gap of the step's alignments, n the segment's length, m
and p the fp64 mass and position: mass within n d + (T_m + 2) 2^-23, position within n^2 d / (2 m) + 2 (T_m + 2) 2^-24 p).
The two preparations of a read (host, device) give scaled tables that may differ in the last place of an f32 element (DESIGN.md section
17); the alignments then move by a few 1e-7, and a position -- a mean over at most 200 samples -- by less than 200 x 200 x 1e-6 / 2 =
0.02 samples: the bound test_read_level holds the two to, where their calls are the same strings; where the two preparations' tables
are the same bytes, it holds the positions and masses to the same bits."""
import ctypes

import numpy as np
import pytest

import gru_reference as G
import longest_output_inputs as I
import moves_reference as M
import signal_map_reference as R
import signal_prep_inputs as SP
from test_parity_gpu import _emitting_flat

pytestmark = pytest.mark.gpu

B, TR, TE, L = 5, 50, 7, 12
FIELDS = M.FIELDS
FILL = R.FILL
# form -> (rnn, mode, attention, decoder cells, options, weight_parts, beam widths)
PER_STEP = dict(persistent_decode=0, use_graph=0)
FORMS = {
    "persistent": ("bilstm", "joint", "luong", 1, {}, 2, (1, 3, 5)),
    "bahdanau": ("bilstm", "joint", "bahdanau", 1, {}, 2, (1, 3, 5)),
    "two_cells": ("bilstm", "joint", "luong", 2, {}, 2, (1, 3, 5)),
    "per_step": ("bilstm", "joint", "luong", 1, PER_STEP, 2, (1, 3, 5)),
    "per_step_graph": ("bilstm", "joint", "luong", 1, dict(PER_STEP, use_graph=1), 2, (1, 3, 5)),
    "weight_parts1": ("bilstm", "joint", "luong", 1, {}, 1, (1, 3, 5)),      # (beam 3 has no one-part form: the two-part kernel on the zero-lo images)
    "gru_per_step": ("bigru", "joint", "luong", 1, {}, 2, (1, 3, 5)),
    "gru_persistent": ("bigru", "joint", "luong", 1, dict(gru_persistent=1), 2, (1, 3, 5)),
    "raw": ("bilstm", "raw", "luong", 1, {}, 2, (5,)),
    "event": ("bilstm", "event", "luong", 1, {}, 2, (5,)),
}
LENS = {"joint": (TR, TE), "raw": (57, 0), "event": (0, 33)}
ENDING = (35, 1.0)          # (weight seed, end-token bias) of _emitting_flat: see test_calls_with_positions


def _slab(mode, seed=3):
    Tr, Te = LENS[mode]
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((B, max(Tr, 1), 1)).astype(np.float32)
    ev = rng.standard_normal((B, max(Te, 1), 5)).astype(np.float32)
    raw[3, raw.shape[1] // 2:] = 0.0
    ev[3, ev.shape[1] // 2:] = 0.0
    raw[4], ev[4] = 0.0, 0.0
    return raw, ev


def _x(mode, raw, ev):
    return {"joint": (raw, ev), "raw": raw, "event": ev}[mode]


def _make(rv, rnn, mode, attention, D, opts, parts, Lmax=L, max_batch=B, seed=22, end_bias=-1.0, Tr=None, Te=None):
    Tr0, Te0 = LENS[mode]
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=2, decoder_depth=D, rnn_type=rnn,
                       attention_type=attention, honor_attention_type=True, max_batch=max_batch, max_raw_len=Tr or max(Tr0, 1),
                       max_event_len=Te or max(Te0, 1), max_output_len=Lmax)
    flat = _emitting_flat(rv, bc.cfg, seed=seed, end_bias=end_bias)
    if parts == 1:
        bc.set_option("weight_parts", 1)
    bc.set_weights_flat(flat)
    for k, v in opts.items():
        bc.set_option(k, v)
    return bc, flat


_BCS = {}


@pytest.fixture(scope="module")
def forms(rv):
    def get(name):
        if name not in _BCS:
            rnn, mode, attention, D, opts, parts, _ = FORMS[name]
            _BCS[name] = _make(rv, rnn, mode, attention, D, opts, parts)
        return _BCS[name]
    yield get
    for bc, _ in _BCS.values():
        bc.close()
    _BCS.clear()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check_calls_moves(bc, x, W, Lc, tag, padding_chunk=True):
    """One calls-with-positions call against the calls call and the moves call on the same inputs -> figures for non-vacuity.
    padding_chunk: the slab's last chunk is padding from end to end, and is held to the NaN rule."""
    steps = Lc - 1
    bases, probs, lens = bc.beam_search_call_arrays(x, W, Lc)
    S0 = bc.last_steps
    b2, p2, l2, mv = bc.beam_search_calls_moves(x, W, Lc)
    assert bc.last_steps == S0 and b2.tobytes() == bases.tobytes() and p2.tobytes() == probs.tobytes() and l2.tobytes() == lens.tobytes(), \
        (tag, "bases / lengths / probs / S differ from the calls call")
    hyp, full = bc.beam_search_moves(x, W, Lc)
    tok = hyp.tokens.numpy()[:, :, 0]
    S = tok.shape[1]
    assert S == S0, (tag, S, S0)
    hlen = hyp.lengths.numpy()[:, 0]
    nB = tok.shape[0]
    dropped = differs = short = 0
    for k in FIELDS:
        got = getattr(mv, k)
        assert got.shape == (nB, steps), (tag, k, got.shape)
        want = bc.base_positions(tok, np.ascontiguousarray(getattr(full, k).numpy()[:, :, 0]))
        for b in range(nB):
            n = int(lens[b])
            assert len(want[b]) == n, (tag, k, b, "letters of the moves call", len(want[b]), n)
            assert np.array_equal(_bits(got[b, :n]), _bits(want[b])), (tag, k, b, got[b, :n].tolist(), want[b].tolist())
            assert (got[b, n:] == FILL[k]).all(), (tag, k, b, "tail", got[b, n:].tolist())
    letters = bc.base_positions(tok, np.broadcast_to(np.arange(S), tok.shape))      # the columns of the kept letters
    for b in range(nB):
        n = int(lens[b])
        short += n < S
        dropped += n > 0 and int(letters[b][-1]) != n - 1                           # a token was dropped before the last kept letter
        pos = mv.raw_pos[b, :n] if (mv.raw_mass[b, :n] > 0).any() else mv.event_pos[b, :n]
        differs += n > 1 and bool((np.diff(pos) != 0).any())
    if not padding_chunk:
        return dict(short=short, dropped=dropped, differs=differs, n4=0, lens=lens.tolist(), S=S)
    # the all-padding chunk: NaN in the five float outputs, -1 in peak, at the letters it holds (its tail: the fill values, above)
    n4 = int(lens[nB - 1])
    nan4 = all(np.isnan(getattr(mv, k)[nB - 1, :n4]).all() for k in FIELDS if k != "peak") and (mv.peak[nB - 1, :n4] == -1).all()
    assert nan4, (tag, "the NaN rule of an all-padding chunk")
    own = np.arange(S)[None, :] < hlen[:, None]
    assert np.isnan(full.raw_mass.numpy()[nB - 1, :, 0][own[nB - 1]]).all(), (tag, "chunk 4 is not padding from end to end")
    return dict(short=short, dropped=dropped, differs=differs, n4=n4, lens=lens.tolist(), S=S)


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("form", list(FORMS))
def test_calls_with_positions(rv, forms, form):
    rnn, mode, attention, D, opts, parts, widths = FORMS[form]
    bc, flat = forms(form)
    raw, ev = _slab(mode)
    x = _x(mode, raw, ev)
    tot = dict(short=0, dropped=0, differs=0)
    try:
        # two sets of weights: long strings (the handle's own), and strings that end inside the row (ENDING: searched on the fp64
        # oracle for the Luong one-cell model, where beams 1 and 3 end chunks 0, 2 and 3 after 5 to 9 letters)
        for wname, wflat in (("long", flat), ("ending", _emitting_flat(rv, bc.cfg, seed=ENDING[0], end_bias=ENDING[1]))):
            bc.set_weights_flat(wflat)
            for W in widths:
                r = _check_calls_moves(bc, x, W, L, f"{form} {wname} W={W}")
                print(f"{form} {wname} W={W}: S = {r['S']}, letters per chunk {r['lens']}, chunks shorter than S {r['short']}, with a token "
                      f"dropped before the last letter {r['dropped']}, whose neighbouring letters differ in position {r['differs']}, letters "
                      f"of the padding chunk {r['n4']}")
                for k in tot:
                    tot[k] += r[k]
        assert tot["short"] + tot["dropped"] > 0 and tot["differs"] > 0, (form, "vacuous", tot)
    finally:
        bc.set_weights_flat(flat)
    # a table that gives EVERY token a letter: nothing is dropped, so element i is column i of the moves call for i < S -- the columns
    # behind a hypothesis's end and the NaN of the all-padding chunk included
    W = widths[-1]
    Tr, Te = LENS[mode]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lut = np.arange(65, 73, dtype=np.uint8)
    bases, lens, probs = np.zeros((B, L - 1), np.uint8), np.zeros(B, np.int32), np.zeros((B, L - 1), np.float32)
    bufs = [np.full((B, L - 1), 0x7F7F7F7F, np.int32).view(np.int32 if k == "peak" else np.float32) for k in FIELDS]
    st = rv._capi.CRvCallMoves(*[p(a) for a in bufs])
    S = ctypes.c_int32(-1)
    bc._check(bc._lib.rv_beam_search_calls_moves(bc._h, p(raw) if Tr else None, p(ev) if Te else None, B, Tr, Te, W, L, p(lut), p(bases), p(lens),
                                                 p(probs), ctypes.byref(st), ctypes.byref(S)), "rv_beam_search_calls_moves")
    hyp, full = bc.beam_search_moves(x, W, L)
    assert (lens == S.value).all() and hyp.tokens.shape[1] == S.value, (form, lens.tolist(), S.value)
    for k, got in zip(FIELDS, bufs):
        ref = np.ascontiguousarray(getattr(full, k).numpy()[:, :, 0])
        assert np.array_equal(_bits(got[:, :S.value]), _bits(ref)), (form, k, "every token kept")
        assert (got[:, S.value:] == FILL[k]).all(), (form, k, "tail")
    own = np.arange(S.value) < int(hyp.lengths.numpy()[B - 1, 0])
    assert own.any() and np.isnan(bufs[0][B - 1, :S.value][own]).all() and (bufs[4][B - 1, :S.value][own] == -1).all(), (form, "the NaN rule")


# ---------------------------------------------------------------------------------------------- 2
def test_longest_output_single_step_and_empty(rv, forms):
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=6, max_raw_len=40, max_event_len=8,
                       max_output_len=I.L, max_beam=8)
    try:
        worst = 0
        for name, W in (("long", 5), ("ragged", 1)):      # (the "ragged" inputs spread the finishing steps at beam 1)
            bc.set_weights_flat(I.flat_weights(rv, bc.cfg, name))
            raw, ev = I.slab(rv, name)
            r = _check_calls_moves(bc, (raw, ev), W, I.L, f"L=64 {name}", padding_chunk=False)
            worst = max(worst, max(r["lens"]))
            print(f"L = 64 {name} W={W}: S = {r['S']}, letters per chunk {r['lens']}")
            if name == "long":
                assert r["S"] == I.STEPS, "the inputs proven to run all 63 steps"
        assert worst > I.HALF, ("no row reaches the second half of the lane = step wave", worst)
    finally:
        bc.close()
    bc, _ = forms("persistent")
    raw, ev = _slab("joint")
    for opts in ({}, PER_STEP):
        for k, v in dict(dict(persistent_decode=1, use_graph=1), **opts).items():
            bc.set_option(k, v)
        _check_calls_moves(bc, (raw, ev), 5, 2, f"L=2 {opts}")
        b0, p0, l0, m0 = bc.beam_search_calls_moves((raw[:0], ev[:0]), 5, L)
        assert b0.shape == (0, L - 1) and all(a.shape == (0, L - 1) for a in m0)
        b1, p1, l1, m1 = bc.beam_search_calls_moves((raw, ev), 5, 1)
        assert b1.shape == (B, 0) and (l1 == 0).all() and all(a.shape == (B, 0) for a in m1)
    for k, v in dict(persistent_decode=1, use_graph=1).items():
        bc.set_option(k, v)


def test_decode_split_parts(rv):
    """The per-step decode of 64 chunks and more runs as `decode_split` sub-slabs, and the finalize kernels once per part, each on its
    part's tokens, records and S: two parts give the bytes of one, with and without the decode graph, and those of the other calls."""
    nB, W = 70, 3            # (on the fp64 oracle the ENDING weights give calls of 3 to 11 letters here, none beyond 9 in the second part)
    bc, _ = _make(rv, "bilstm", "joint", "luong", 1, dict(PER_STEP, decode_split=1), 2, max_batch=nB, seed=ENDING[0], end_bias=ENDING[1])
    try:
        raw, ev, _ = rv.synthetic.make_slab(nB, TR, TE, seed=8)
        one = bc.beam_search_calls_moves((raw, ev), W, L)
        assert len(set(one[2].tolist())) >= 3, ("the chunks' calls all have one length", sorted(set(one[2].tolist())))
        for graph in (0, 1):
            bc.set_option("use_graph", graph)
            bc.set_option("decode_split", 2)
            r = _check_calls_moves(bc, (raw, ev), W, L, f"decode_split 2 use_graph {graph}", padding_chunk=False)
            two = bc.beam_search_calls_moves((raw, ev), W, L)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(two[:3], one[:3])) and \
                all(a.tobytes() == b.tobytes() for a, b in zip(two[3], one[3])), f"decode_split 2 use_graph {graph}: not the bytes of one part"
        print(f"decode_split 2: S = {r['S']}, distinct call lengths {sorted(set(r['lens']))}, chunks shorter than S {r['short']}")
    finally:
        bc.close()


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("form", ["persistent", "per_step", "gru_per_step"])
def test_window_calls(rv, forms, form):
    bc, _ = forms(form)
    rng = np.random.default_rng(5)
    raw_sc = rng.standard_normal(400).astype(np.float32)
    ev_sc = rng.standard_normal((60, 5)).astype(np.float32)
    win = np.array([[0, 50, 0, 7], [30, 41, 5, 7], [100, 50, 12, 3], [151, 17, 20, 7], [349, 50, 53, 7], [200, 1, 30, 1], [7, 50, 9, 6],
                    [250, 33, 40, 7], [90, 50, 1, 7], [300, 49, 50, 2], [10, 10, 10, 7], [390, 10, 58, 2]], np.int32)
    h = bc.put_read(raw_sc, ev_sc)
    try:
        slabs = [win[0:5], win[5:9], win[9:12]]
        want = []
        for w in slabs:
            raw, ev = rv.data_loader.expand_windows(raw_sc, ev_sc, w, TR, TE)
            want.append(bc.beam_search_calls_moves((raw, ev), 5, L))
        same = lambda got, ref: all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], ref[:3])) and \
            all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(got[3], ref[3]))
        for w, ref in zip(slabs, want):
            assert same(bc.beam_search_windows_calls_moves(h.table(w), 5, L, T_r=TR, T_e=TE), ref), (form, "synchronous window call")
        # three slabs through depth 2
        bc.set_async_depth(2)
        got = list(bc.beam_search_stream_windows((h.table(w) for w in slabs), 5, L, calls=True, T_r=TR, T_e=TE, moves=True))
        assert len(got) == 3 and all(same(g, r) for g, r in zip(got, want)), (form, "asynchronous window calls")
        # tickets collected out of order; the wrong collect leaves the ticket in flight
        t0 = bc.submit_windows(h.table(slabs[0]), 5, L, calls=True, T_r=TR, T_e=TE, moves=True)
        t1 = bc.submit_windows(h.table(slabs[1]), 5, L, calls=True, T_r=TR, T_e=TE, moves=True)
        with pytest.raises(rv._capi.RavventHipError, match="RV_EINVAL.*rv_beam_search_collect_calls_moves"):
            bc.collect_calls(t1)
        with pytest.raises(rv._capi.RavventHipError, match="RV_ESTATE"):      # the read is in use
            h.drop()
        assert same(bc.collect_calls_moves(t1), want[1]) and same(bc.collect_calls_moves(t0), want[0]), (form, "out of order")
        plain = bc.submit_windows(h.table(slabs[2]), 5, L, calls=True, T_r=TR, T_e=TE)
        with pytest.raises(rv._capi.RavventHipError, match="RV_EINVAL.*rv_beam_search_submit_windows_calls_moves"):
            bc.collect_calls_moves(plain)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(bc.collect_calls(plain), want[2][:3]))
    finally:
        h.drop()


# ---------------------------------------------------------------------------------------------- 4
FORCED = ["persistent", "per_step", "two_cells", "gru_per_step", "gru_persistent", "bahdanau"]


def _targets(cfg, seed=9):
    rng = np.random.default_rng(seed)
    t = rng.integers(3, 7, (B, L)).astype(np.int32)
    t[:, 0] = cfg.start_token
    t[0, 8] = cfg.end_token
    t[0, 9:] = cfg.pad_token                 # padding labels behind an end token
    t[1, 5] = cfg.pad_token                  # ... and one inside a row
    t[2, L - 1] = cfg.end_token
    return t


@pytest.mark.parametrize("form", FORCED)
def test_forced_moves(rv, oracle, forms, form):
    import torch
    rnn, mode, attention, D, opts, parts, _ = FORMS[form]
    bc, flat = forms(form)
    raw, ev = _slab(mode)
    tg = _targets(bc.cfg)
    Tm, steps = TR + TE, L - 1
    persist = form in ("persistent", "two_cells", "gru_persistent", "bahdanau")
    # the existing calls' bytes
    sid, lg = bc.teacher_forced_prediction((raw, ev), tg)
    nll, nsum = bc.sequence_nll((raw, ev), tg)
    tap = "persist_taps" if persist else "debug_taps"
    sc, mv = bc.align((raw, ev), tg)
    for k, a in (("sample_id", sid), ("logits", lg), ("nll", nll), ("nll_sum", nsum)):
        assert getattr(sc, k).numpy().tobytes() == a.numpy().tobytes(), (form, k, "differs from the call without moves")
    assert all(tuple(a.shape) == (B, steps) for a in mv), form
    mvn = {k: getattr(mv, k).numpy() for k in FIELDS}
    # the device variant: the same bits
    dev = tuple(torch.from_numpy(a.copy()).cuda() for a in (raw, ev))
    dsc, dmv = bc.align(dev, torch.from_numpy(tg).cuda())
    assert all(t.is_cuda for t in dmv)
    for k in FIELDS:
        assert np.array_equal(_bits(getattr(dmv, k).cpu().numpy()), _bits(mvn[k])), (form, k, "device variant")
    assert dsc.logits.cpu().numpy().tobytes() == lg.numpy().tobytes() and dsc.nll.cpu().numpy().tobytes() == nll.numpy().tobytes()
    # padding labels: the fill values
    padl = tg[:, 1:] == bc.cfg.pad_token
    assert padl.sum() >= 3
    for k in FIELDS:
        assert (mvn[k][padl] == FILL[k]).all(), (form, k, "padding labels")
    # the all-padding chunk: NaN, no peak
    assert all(np.isnan(mvn[k][4]).all() for k in FIELDS if k != "peak") and (mvn["peak"][4] == -1).all(), (form, "NaN rule")
    # against fp64, d from the form's own alignment tap
    bc.set_option(tap, 1)
    try:
        sc2, mv2 = bc.align((raw, ev), tg)
        al32 = bc.get_tensor("step_alignments").reshape(steps, B, 1, Tm)[:, :, 0].transpose(1, 0, 2).astype(np.float64)
    finally:
        bc.set_option(tap, 0)
    if persist:      # (debug_taps moves a call to the per-step kernels; persist_taps keeps the form)
        for k in FIELDS:
            assert np.array_equal(_bits(getattr(mv2, k).numpy()), _bits(mvn[k])), (form, k, "the tap changed the moves")
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    ref, a64 = R.forced_moves(oracle, w, bc.cfg.oracle_cfg(), raw, ev, tg, TR, bc.cfg.pad_token, gru=G if rnn == "bigru" else None)
    u, worst_d, checked, apart = 2.0 ** -24, 0.0, 0, 0
    for b in range(4):
        for t in range(steps):
            if padl[b, t]:
                continue
            d = float(np.abs(al32[b, t] - a64[b, t]).max())
            worst_d = max(worst_d, d)
            assert d <= 1e-4, (form, b, t, "alignments", d)
            for seg, n in (("raw", TR), ("event", TE)):
                m64, p64 = ref[seg + "_mass"][b, t], ref[seg + "_pos"][b, t]
                mg, pg = float(mvn[seg + "_mass"][b, t]), float(mvn[seg + "_pos"][b, t])
                if m64 == 0:
                    assert mg == 0 and pg == -1 and p64 == -1, (form, b, t, seg, "an exactly zero mass")
                    continue
                assert mg != 0 and abs(mg - m64) <= n * d + (Tm + 2) * 2 * u, (form, b, t, seg, "mass", mg, m64, d)
                tol = n * n * d / (2 * m64) + 2 * (Tm + 2) * u * p64
                assert abs(pg - p64) <= tol, (form, b, t, seg, "pos", pg, p64, tol, d)
                checked += 1
                if seg == "raw" and t > 0 and not padl[b, t - 1] and ref["raw_mass"][b, t - 1] > 0:
                    apart += abs(ref["raw_pos"][b, t - 1] - p64) > 4 * tol
            pk = int(mvn["peak"][b, t])
            assert 0 <= pk < Tm and a64[b, t, pk] >= a64[b, t].max() - 2 * d, (form, b, t, "peak", pk)
    print(f"{form}: max |alpha - fp64| = {worst_d:.2e}, positions checked {checked}, neighbouring steps told apart by 4 x tolerance {apart}")
    assert checked >= 40 and apart > 0, (form, "vacuous", checked, apart)


@pytest.mark.parametrize("form", ["persistent", "bahdanau", "two_cells", "gru_persistent"])
def test_forced_on_the_beam_one_tokens_is_the_beam_one_call(rv, forms, form):
    """Both decodes run the W = 1 instantiation of the persistent kernel on the same inputs: a forced call fed [start] + the beam-1
    call's tokens returns that call's moves bit for bit up to each chunk's length."""
    rnn, mode, attention, D, opts, parts, _ = FORMS[form]
    bc, _ = forms(form)
    raw, ev = _slab(mode)
    hyp, mv = bc.beam_search_moves((raw, ev), 1, L)
    tok, ln = hyp.tokens.numpy()[:, :, 0], hyp.lengths.numpy()[:, 0]
    S = tok.shape[1]
    tg = np.full((B, L), bc.cfg.pad_token, np.int32)
    tg[:, 0] = bc.cfg.start_token
    tg[:, 1:S + 1] = tok
    _, fm = bc.align((raw, ev), tg)
    n_cmp = 0
    for k in FIELDS:
        a, f = getattr(mv, k).numpy()[:, :, 0], getattr(fm, k).numpy()
        for b in range(B):
            n = min(int(ln[b]), S)
            lab = tg[b, 1:n + 1] != bc.cfg.pad_token
            assert np.array_equal(_bits(np.ascontiguousarray(f[b, :n][lab])), _bits(np.ascontiguousarray(a[b, :n][lab]))), \
                (form, k, b, f[b, :n].tolist(), a[b, :n].tolist())
            n_cmp += int(lab.sum())
    assert n_cmp >= 6 * 12, (form, "columns compared", n_cmp)


# ---------------------------------------------------------------------------------------------- 5
_READ = {}


def _chunk_level(bc, mode, raw_sc, ev_sc, windows, W, Lr):
    """Per chunk the positions of its letters from separate beam_search_moves calls on the expanded chunks."""
    T_r, T_e = 200, 30
    out = {k: [] for k in ("raw_pos", "raw_mass", "event_pos", "event_mass")}
    for a in range(0, len(windows), 16):
        raw, ev = rv_expand(raw_sc, ev_sc, windows[a:a + 16], T_r, T_e)
        hyp, mv = bc.beam_search_moves(_x(mode, raw, ev), W, Lr)
        tok = hyp.tokens.numpy()[:, :, 0]
        for k in out:
            out[k] += bc.base_positions(tok, np.ascontiguousarray(getattr(mv, k).numpy()[:, :, 0]))
    return out


def rv_expand(raw_sc, ev_sc, windows, T_r, T_e):
    import ravvent_basecaller_amd as rv
    return rv.data_loader.expand_windows(raw_sc, ev_sc, windows, T_r, T_e)


@pytest.mark.parametrize("mode", ["raw", "joint", "event"])      # (event mode: the event estimate end to end)
def test_read_level(rv, mode):
    Lr, W = 40, 5            # calls longer than the merger's overlap of 25, so that the merged read grows with every chunk
    sig = np.asarray(SP.synthetic_signal(rv, 500, 11)).astype(np.int16)
    assert 3000 <= len(sig) <= 6000
    bc, _ = _make(rv, "bilstm", mode, "luong", 1, {}, 2, Lmax=Lr, max_batch=16, Tr=200, Te=30)
    try:
        res, tables = {}, {}
        for dev in (False, True):
            plain = bc.basecall(sig, max_output_len=Lr, chunk_size=16, device_prep=dev)
            r = bc.basecall(sig, max_output_len=Lr, chunk_size=16, device_prep=dev, moves=True)
            tag = (mode, "device_prep", dev)
            assert plain.positions is None and plain.source_chunk is None
            assert r.seq == plain.seq and r.probs.tobytes() == plain.probs.tobytes() and r.chunks_num == plain.chunks_num, (tag, "seq / probs")
            n = len(r.seq)
            assert r.positions.dtype == np.float64 and all(len(a) == n for a in (r.positions, r.raw_mass, r.event_mass, r.source_chunk, r.source_index))
            # the tables and events of this preparation
            if dev:
                h = bc.put_signal(sig, stride=6, max_raw_len=200, max_event_len=30)
                raw_sc, ev_sc, windows = h.fetch("raw_sc"), h.fetch("events_sc"), h.windows
                st, ln = h.fetch("start"), h.fetch("length")
                h.drop()
            else:
                rw = rv.data_loader.prepare_windows(sig, stride=6)
                raw_sc, ev_sc, windows = rw.raw_sc, rw.events_sc, rw.windows
                st, ln, _, _ = rv.event_detection.EventDetector(window_length1=rv.data_loader.ED_WINDOW_LENGTH_1,
                                                                 window_length2=rv.data_loader.ED_WINDOW_LENGTH_2).run_arrays(sig)
            assert len(windows) == r.chunks_num
            cl = _chunk_level(bc, mode, raw_sc, ev_sc, windows, W, Lr)
            ck, ix = r.source_chunk, r.source_index
            g = lambda k: np.array([cl[k][c][i] for c, i in zip(ck, ix)])
            want = rv.basecaller.signal_positions(mode, windows[ck, 0], windows[ck, 2], g("raw_pos"), g("raw_mass"), g("event_pos"),
                                                  g("event_mass"), st, ln)
            assert np.array_equal(want.view(np.uint64), r.positions.view(np.uint64)), (tag, "positions are not the formula on the chunk-level values")
            assert np.array_equal(_bits(g("raw_mass").astype(np.float32)), _bits(r.raw_mass)) and \
                np.array_equal(_bits(g("event_mass").astype(np.float32)), _bits(r.event_mass)), (tag, "masses")
            ok = ~np.isnan(r.positions)
            assert ok.any() and (r.positions[ok] >= 0).all() and (r.positions[ok] < len(sig)).all(), (tag, "a position outside the signal")
            assert n >= 50 and len(set(ck.tolist())) >= 5, (tag, "vacuous", n, len(set(ck.tolist())))
            if mode == "joint":
                took_raw = r.raw_mass >= r.event_mass
                print(f"{tag}: bases {n}, from {len(set(ck.tolist()))} chunks, raw estimate taken for {int(took_raw.sum())}")
            lines = r.positions_tsv("read").splitlines()
            assert lines[0] == "# read" and len(lines) == n + 1 and lines[1].split("\t")[:2] == ["0", r.seq[0]]
            res[dev], tables[dev] = r, (raw_sc, ev_sc)
        a, b = res[False], res[True]
        assert a.seq == b.seq and np.array_equal(a.source_chunk, b.source_chunk) and np.array_equal(a.source_index, b.source_index), \
            (mode, "the two preparations call different reads")
        gap = np.nanmax(np.abs(a.positions - b.positions))
        print(f"{mode}: the two preparations' positions differ by at most {gap:.3g} samples")
        assert np.array_equal(np.isnan(a.positions), np.isnan(b.positions)) and gap <= 0.02, (mode, gap)
        if all(x.tobytes() == y.tobytes() for x, y in zip(tables[False], tables[True])):      # the same tables: the same bits
            assert np.array_equal(a.positions.view(np.uint64), b.positions.view(np.uint64)), (mode, "equal tables, other positions")
            assert a.raw_mass.tobytes() == b.raw_mass.tobytes() and a.event_mass.tobytes() == b.event_mass.tobytes(), mode
        many = bc.basecall_many([sig, sig[:1500]], max_output_len=Lr, chunk_size=16, moves=True)
        assert many[0].seq == a.seq and np.array_equal(many[0].positions.view(np.uint64), a.positions.view(np.uint64)), "basecall_many"
        assert many[1].positions is not None and len(many[1].positions) == len(many[1].seq)
    finally:
        bc.close()


# ---------------------------------------------------------------------------------------------- 6
def test_refusals(rv, forms):
    bc, _ = forms("persistent")
    raw, ev = _slab("joint")
    err = rv._capi.RavventHipError
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lut = bc._call_lut()
    bases, lens, probs = np.zeros((B, L - 1), np.uint8), np.zeros(B, np.int32), np.zeros((B, L - 1), np.float32)
    S = ctypes.c_int32(-1)
    none = rv._capi.CRvCallMoves()
    rc = bc._lib.rv_beam_search_calls_moves(bc._h, p(raw), p(ev), B, TR, TE, 5, L, p(lut), p(bases), p(lens), p(probs), ctypes.byref(none),
                                            ctypes.byref(S))
    assert rc == -1 and b"null output pointer" in bc._lib.rv_last_error(bc._h)
    tg = _targets(bc.cfg)
    sid, lg = np.zeros((B, L - 1), np.int32), np.zeros((B, L - 1, bc.cfg.vocab), np.float32)
    nomv, nosc = rv._capi.CRvMoves(), rv._capi.CRvScore()
    rc = bc._lib.rv_teacher_forced_moves(bc._h, p(raw), p(ev), B, TR, TE, L, p(tg), 0, p(sid), p(lg), ctypes.byref(nosc), ctypes.byref(nomv))
    assert rc == -1 and b"null output pointer" in bc._lib.rv_last_error(bc._h)
    # one member alone is enough, and the others are not touched
    one = np.full((B, L - 1), 7, np.float32)
    only = rv._capi.CRvCallMoves(raw_pos=p(one))
    bc._check(bc._lib.rv_beam_search_calls_moves(bc._h, p(raw), p(ev), B, TR, TE, 5, L, p(lut), p(bases), p(lens), p(probs), ctypes.byref(only),
                                                 ctypes.byref(S)), "rv_beam_search_calls_moves")
    full = bc.beam_search_calls_moves((raw, ev), 5, L)
    assert np.array_equal(_bits(one), _bits(full[3].raw_pos)) and bases.tobytes() == full[0].tobytes()
    # the limits, by their existing messages
    with pytest.raises(err, match=r"RV_EINVAL: max_output_len=13 outside \[1,12\]"):
        bc.beam_search_calls_moves((raw, ev), 5, L + 1)
    with pytest.raises(err, match=r"RV_EINVAL: max_output_len=13 outside \[1,12\]"):
        bc.align((raw, ev), np.concatenate([tg, tg[:, :1]], axis=1))
    with pytest.raises(err, match=r"RV_EINVAL: beam width 9 outside"):
        bc.beam_search_calls_moves((raw, ev), 9, L)
    with pytest.raises(err, match=r"RV_EINVAL: target id 7 at \[1,2\] outside \[0,7\)"):
        bad = tg.copy()
        bad[1, 2] = 7
        bc.align((raw, ev), bad)
    wide = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=2, max_raw_len=340, max_event_len=20, max_output_len=4)
    try:
        wide.init_random_weights(seed=1)
        r2, e2, _ = rv.synthetic.make_slab(2, 340, 20, seed=1)
        with pytest.raises(err, match="RV_EUNSUPPORTED: attention memory of 360 steps exceeds the 352"):
            wide.beam_search_calls_moves((r2, e2), 3, 4)
        with pytest.raises(err, match="RV_EUNSUPPORTED: attention memory of 360 steps exceeds the 352"):
            wide.align((r2, e2), np.full((2, 4), 3, np.int32))
    finally:
        wide.close()
    # a synchronous call while every context holds a ticket: RV_ESTATE, nothing touched; the handle works afterwards
    rng = np.random.default_rng(2)
    h = bc.put_read(rng.standard_normal(100).astype(np.float32), rng.standard_normal((20, 5)).astype(np.float32))
    try:
        bc.set_async_depth(2)
        tab = h.table(np.array([[0, 50, 0, 7], [40, 50, 10, 7]], np.int32))
        t0 = bc.submit_windows(tab, 5, L, calls=True, T_r=TR, T_e=TE, moves=True)
        t1 = bc.submit_windows(tab, 5, L, calls=True, T_r=TR, T_e=TE, moves=True)
        for call in (lambda: bc.beam_search_calls_moves((raw, ev), 5, L), lambda: bc.align((raw, ev), tg),
                     lambda: bc.submit_windows(tab, 5, L, calls=True, T_r=TR, T_e=TE, moves=True)):
            with pytest.raises(err, match="RV_ESTATE"):
                call()
        r1, r0 = bc.collect_calls_moves(t1), bc.collect_calls_moves(t0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r0[:3], r1[:3])) and all(a.tobytes() == b.tobytes() for a, b in zip(r0[3], r1[3]))
    finally:
        h.drop()
    again = bc.beam_search_calls_moves((raw, ev), 5, L)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], full[:3])) and all(a.tobytes() == b.tobytes() for a, b in zip(again[3], full[3]))
