"""Every decode output at max_output_len = 64, the library's limit: 63 steps, the length a family of code is written against.

k_dec_finalize (decode.hip) runs one wave with lane = step over s_tok[64], compacts letters with a 64-bit ballot and takes probabilities
from the neighbouring lane; k_dec_finalize_beams (beams.hip) and k_dec_finalize_moves (moves.hip) keep [64 * RV_MAX_BEAM] LDS arrays
indexed t * W + w; k_dec_reduce_steps uses lane = step; k_score_tokens (score.hip) lane = position; the records [S,B,W], step_moves
[S,B,W,6] and the host staging of max_batch x max_output_len x max_beam exist at their full size only at L = 64 and W = 8.  The tests
here hold each of those outputs to its records, exactly, and to the fp64 oracle, at the smallest shapes that reach the limit.

Shapes: the B = 6 chunks of test_kernel_forms_gpu._slab("joint", 40, 8, seed) (T_m = 48, NIT 2), L = 64, beams 1, 5 and 8 (two decoder
cells: 5), handles of max_output_len 64 and max_beam 8; shape C: chunks 1 and 2 of the same slab at T_m = 308 + 44 = 352 (NIT 11),
W = 5, for the moves and the whole beam; the decode_split form on a slab of 70 chunks from synthetic.make_slab (a slab is split from 64
chunks on).

Inputs (longest_output_inputs.py).  All weights are test_parity_gpu._emitting_flat(seed, end_bias); they were searched on the CPU with
oracle.beam_search in fp64 and its numpy fp32 twin, upwards from the first pair tried, for the first at which the twin returns the
fp64 step ids and parents on EVERY chunk for all 63 steps with scores within 4e-5 of fp64 (so that test_parity_gpu._assert_twin's
2 x twin + 5e-6 stays below 1e-4) and the records are not vacuous (tests/test_longest_output.py asserts all of it without a GPU):
  "long"    weight seed 22, end bias -1.0, slab seed 1: every hypothesis of every chunk runs all 63 steps; parents that are not the
            identity at steps >= 32: 528 at W = 8, 241 at W = 5 (Luong, one cell), some at steps >= 56, and hypotheses w > 0 differ from
            hypothesis 0 in columns >= 32 -- a back-trace that is wrong only when it is deep, or only in the upper half of the wave.
  "spread"  weight seed 22, end bias 1.5, slab seed 1: the chunks' beams are all finished at [63, 13, 63, 12, 15, 63] (Luong, W = 8),
            [63, 14, 63, 14, 15, 63] (W = 5), [63, 14, 63, 11, 15, 63] (Bahdanau, W = 5), [3, 5, 3, 63, 11, 63] (two cells); hypothesis 0
            ends at its first step everywhere.  At W = 1 these weights end five chunks at step 1, so the W = 1 cases take "ragged".
  "ragged"  weight seed 24, end bias 1.0, slab seed 1, W = 1: best-hypothesis lengths [63, 63, 63, 9, 8, 9], letters [63, 58, 63, 8, 7, 8]
            (Luong; Bahdanau 57 in chunk 1): two 63-letter rows, and chunk 1 holds non-letter ids between its letters, which the
            compaction has to skip.  (Seed 23, the first tried, has its non-letter ids only behind the last letter of a row.)  The greedy
            search runs all 63 steps on the six chunks and 9 on chunks 3 .. 5 alone.
  shape C   slab seed 1, chunks 1 and 2 of the six: on "long" chunk 2 changes slots after step 56, on "spread" chunk 1 runs 63 steps and
            chunk 2 is finished after 17 (on "spread" chunks 2 and 3, the first pair looked at, keep the best path in slot 0 throughout; with all
            six chunks the twin's scores on "long" are 8.4e-5 from fp64, chunk 4 alone).
  B = 70    "long": slab seed 8 (at seeds 1 .. 7 the twin leaves the fp64 decode on one chunk of the 70), "spread": slab seed 2 (at
            seed 1 it leaves on chunk 2).
The tests assert the conditions again on the GPU's own records before they rely on them."""
import ctypes

import numpy as np
import pytest

import longest_output_inputs as I
import moves_reference as M
from test_beams_gpu import _assert_equal, _assert_not_vacuous, _bits, _expect, _host_bufs, _np_beams, _records, _stats
from test_config_space_gpu import _beam_entry_points, _calls_entry_points, _filled, _greedy_entry_points, _no_sentinel
from test_kernel_forms_gpu import PERSIST, _decode_forms, _handle, _set, _x
from test_moves_gpu import _move_bufs, _np_moves
from test_parity_gpu import _assert_twin
from test_teacher_forced import np_counts, np_nll

pytestmark = pytest.mark.gpu

L, STEPS, TOL = I.L, I.STEPS, 1e-4
MX = dict(matrix_attention=1, matrix_cell=1)
PERSIST_OPTS = dict(persistent_decode=1, use_graph=1, decode_split=1, **MX)
# form -> (family of longest_output_inputs, options, the ATT of k_dec_persist it must run or None for the per-step kernels, beam
#          widths, on the slab of 70 chunks)
FORMS = {
    "persistent": ("luong1", PERSIST_OPTS, 3, (1, 5, 8), False),
    "bahdanau": ("bahdanau1", PERSIST_OPTS, 4, (1, 5, 8), False),
    "two_cells": ("luong2", PERSIST_OPTS, 3, (5,), False),
    "per_step": ("luong1", dict(persistent_decode=0, use_graph=0, decode_split=1, **MX), None, (1, 5, 8), False),
    "per_step_graph": ("luong1", dict(persistent_decode=0, use_graph=1, decode_split=1, **MX), None, (1, 5, 8), False),
    "decode_split": ("luong1", dict(persistent_decode=0, use_graph=0, decode_split=2, **MX), None, (5,), True),
}
NIT = {"A": 2, "C": 11}
CASES = [(f, k, W) for f, spec in FORMS.items() for W in spec[3] for k in ("long", "spread")]
MOVE_CASES = [(f, k, W, "A") for f, k, W in CASES if W > 1] + [(f, k, 5, "C") for f in ("persistent", "per_step_graph") for k in ("long", "spread")]


# ---------------------------------------------------------------------------------------------- handles and results: made once
_HANDLES, _LOADED, _RESULTS, _MOVES = {}, {}, {}, {}


@pytest.fixture(scope="module")
def handles(rv):
    def get(fam, shape="A", split=False):
        key = (fam, shape, split)
        if key not in _HANDLES:
            attention, D, _ = I.FAMILIES[fam]
            TR, TE, _ = I.SHAPES[shape]
            _HANDLES[key] = _handle(rv, "joint", attention, D, 1, Tr_max=TR, Te_max=TE, L=L, max_batch=I.SPLIT_B if split else 6)[0]
        return _HANDLES[key]
    yield get
    for bc in _HANDLES.values():
        bc.close()
    for d in (_HANDLES, _LOADED, _RESULTS, _MOVES):
        d.clear()


def _ready(rv, handles, form, name, shape="A"):
    """The form's handle with the weights of `name` loaded and the form's options set."""
    fam, opts, att, _, split = FORMS[form]
    bc = handles(fam, shape, split)
    if _LOADED.get(id(bc)) != (name, split):
        bc.set_weights_flat(I.flat_weights(rv, bc.cfg, name, split))
        _LOADED[id(bc)] = (name, split)
    _set(bc, opts)
    return bc


def _assert_form(rv, bc, form, W, shape, tag):
    fam, opts, att, _, split = FORMS[form]
    forms = _decode_forms(bc)
    if att is None:
        assert forms and not any(r[0] == PERSIST for r in forms), (tag, sorted(forms))
    else:
        assert {r for r in forms if r[0] == PERSIST} == {(PERSIST, W, NIT[shape], I.FAMILIES[fam][1], att)}, (tag, sorted(forms))
    if opts["decode_split"] > 1:       # the split was in force: its records lie per sub-slab and the library says so
        with pytest.raises(rv._capi.RavventHipError, match="RV_ESTATE.*decode_split"):
            bc.get_tensor("step_ids")


def _own_records(rv, bc, form, x, W, S, nB, call, tag):
    """The records a call left (oracle-free): for the decode_split form those of the same call with decode_split 1, whose outputs
    must be the split call's byte for byte -> (records, the unsplit call's outputs or None)."""
    _, opts, att, _, _ = FORMS[form]
    one = None
    if opts["decode_split"] > 1:
        bc.set_option("decode_split", 1)
        one = call()
        bc.set_option("decode_split", opts["decode_split"])
    return _records(bc, S, nB, W, att is not None), one


def _same_fields(a, b, tag):
    for k in a._fields:
        assert getattr(a, k).shape == getattr(b, k).shape and getattr(a, k).tobytes() == getattr(b, k).tobytes(), (tag, k)


def _result(rv, handles, oracle, form, kind, W, shape="A"):
    """One all-beams call of a form, the expectation from its own records and the oracle passes of its inputs (made once)."""
    key = (form, kind, W, shape)
    if key not in _RESULTS:
        fam, opts, att, _, split = FORMS[form]
        name = I.inputs_for(kind, W)
        tag = f"{form} {name} W={W} {shape}"
        p = I.passes(rv, oracle, fam, name, W, shape, split)
        bc = _ready(rv, handles, form, name, shape)
        x = _x("joint", p["raw"], p["ev"])
        call = lambda: _np_beams(bc.beam_search_hypotheses(x, W, L))
        got = call()
        _assert_form(rv, bc, form, W, shape, tag)
        S, nB = got.tokens.shape[1], p["raw"].shape[0]
        rec, one = _own_records(rv, bc, form, x, W, S, nB, call, tag)
        if one is not None:
            _same_fields(got, one, tag + ": decode_split 2 against 1")
        e = _expect(oracle, *rec, bc.cfg.end_token)
        _RESULTS[key] = (got, e, S, p, name)
    return _RESULTS[key]


def _assert_conditions(e, name, W, tag):
    _assert_not_vacuous(e, W, tag, finish_apart=name != "long")
    if name == "long":
        I.assert_long(e, W, tag)
    else:
        I.assert_spread(e, W, tag)


# ---------------------------------------------------------------------------------------------- 1: the whole beam, exact
@pytest.mark.parametrize("form,kind,W", CASES)
def test_whole_beam_equals_gather_tree_of_the_records(rv, handles, oracle, form, kind, W):
    got, e, S, p, name = _result(rv, handles, oracle, form, kind, W)
    tag = f"{form} {name} W={W}"
    print(f"{tag}: S = {S}, finished at {e['fin_at'].tolist()}, lengths of hypothesis 0 {e['lengths'][:, 0].tolist()}, parents not the "
          f"identity from step 32: {int((e['par'][32:] != np.arange(W)).sum())}")
    assert S == STEPS, (tag, S)
    _assert_conditions(e, name, W, tag)
    _assert_equal(got, e, tag)


# ---------------------------------------------------------------------------------------------- 2: the whole beam against fp64
@pytest.mark.parametrize("form,kind,W", CASES)
def test_whole_beam_against_fp64(rv, handles, oracle, form, kind, W):
    got, e, S, p, name = _result(rv, handles, oracle, form, kind, W)
    tag = f"{form} {name} W={W}"
    o = p["o"]
    assert S == o["ids"].shape[0] == STEPS, (tag, S, o["ids"].shape)
    left = [b for b in range(e["ids"].shape[1]) if (e["ids"][:, b] != o["ids"][:, b]).any() or (e["par"][:, b] != o["par"][:, b]).any()]
    assert not left, (tag, "chunks that left the fp64 decode: the inputs are badly chosen, or the decode is wrong", left)
    assert np.array_equal(got.tokens, o["tokens"]) and np.array_equal(got.lengths, o["lengths"]), (tag, "tokens / lengths")
    err = {k: I.max_error(getattr(got, k), o[k]) for k in ("scores", "path_scores", "log_probs")}
    twin = {k: p["twin"][k] for k in err}
    _assert_twin(err, twin, tag)                     # (prints tensor, GPU error, twin error, ratio)
    assert max(err.values()) < TOL, (tag, err)


# ---------------------------------------------------------------------------------------------- 3: slot 0 is the existing call
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _all_host(rv, bc, raw, ev, W, Lc=L):
    """rv_beam_search_all on sentinel-filled host buffers of the full width -> (the five buffers, S)."""
    bufs, S = _host_bufs(raw.shape[0], W, steps=Lc - 1), ctypes.c_int32(-1)
    st = rv._capi.CRvBeams(*[_p(a) for a in bufs])
    bc._check(bc._lib.rv_beam_search_all(bc._h, _p(raw), _p(ev), raw.shape[0], raw.shape[1], ev.shape[1], W, Lc, ctypes.byref(st), ctypes.byref(S)),
              "rv_beam_search_all")
    return bufs, S.value


def _all_dev(rv, bc, raw, ev, W):
    import torch
    d_raw, d_ev = torch.from_numpy(raw.copy()).cuda(), torch.from_numpy(ev.copy()).cuda()
    like = _host_bufs(raw.shape[0], W, steps=STEPS)
    dbufs = [torch.full(a.shape, 0x7F7F7F7F, dtype=torch.int32, device="cuda") for a in like]
    torch.cuda.synchronize()
    st, S = rv._capi.CRvBeams(*[_dp(t) for t in dbufs]), ctypes.c_int32(-1)
    bc._check(bc._lib.rv_beam_search_all_dev(bc._h, _dp(d_raw), _dp(d_ev), raw.shape[0], raw.shape[1], ev.shape[1], W, L, ctypes.byref(st),
                                             ctypes.byref(S)), "rv_beam_search_all_dev")
    return [t.cpu().numpy().view(a.dtype) for t, a in zip(dbufs, like)], S.value


@pytest.mark.parametrize("form,kind,W", CASES)
def test_slot_zero_is_the_existing_call(rv, handles, oracle, form, kind, W):
    got, e, S, p, name = _result(rv, handles, oracle, form, kind, W)
    tag = f"{form} {name} W={W}"
    bc = _ready(rv, handles, form, name)
    raw, ev = p["raw"], p["ev"]
    bufs, Sh = _all_host(rv, bc, raw, ev, W)
    assert Sh == S == STEPS, (tag, Sh, S)
    _no_sentinel(*bufs)
    for k, a in zip(got._fields, bufs):
        assert a.tobytes() == getattr(got, k).tobytes(), (tag, "rv_beam_search_all on the caller's buffers", k)
    dbufs, Sd = _all_dev(rv, bc, raw, ev, W)
    assert Sd == S and all(d.tobytes() == a.tobytes() for d, a in zip(dbufs, bufs)), (tag, "rv_beam_search_all_dev")
    tok0, sc0 = np.ascontiguousarray(bufs[0][:, :, 0]), np.ascontiguousarray(bufs[1][:, :, 0])
    for entry, tok, sc, Se in _beam_entry_points(bc, raw, ev, W, L=L):
        assert Se == S and tok.shape == (raw.shape[0], STEPS), (tag, entry, Se, tok.shape)
        assert tok.tobytes() == tok0.tobytes(), (tag, entry, "tokens", np.argwhere(tok != tok0)[:5].tolist())
        assert sc.tobytes() == sc0.tobytes(), (tag, entry, "scores")


# ---------------------------------------------------------------------------------------------- 4: the moves
def _moves_result(rv, handles, oracle, form, kind, W, shape):
    key = (form, kind, W, shape)
    if key not in _MOVES:
        fam, opts, att, _, split = FORMS[form]
        name = I.inputs_for(kind, W)
        tag = f"moves {form} {name} W={W} {shape}"
        p = I.passes(rv, oracle, fam, name, W, shape, split)
        bc = _ready(rv, handles, form, name, shape)
        x = _x("joint", p["raw"], p["ev"])

        def call():
            hyp, mv = bc.beam_search_moves(x, W, L)
            return _np_beams(hyp), _np_moves(mv)
        hyp, mv = call()
        _assert_form(rv, bc, form, W, shape, tag)
        S, nB = hyp.tokens.shape[1], p["raw"].shape[0]
        recs, one = _own_records(rv, bc, form, x, W, S, nB, call, tag)
        if one is not None:
            _same_fields(hyp, one[0], tag + ": decode_split 2 against 1")
            _same_fields(mv, one[1], tag + ": decode_split 2 against 1")
        moves_rec = bc.get_tensor("step_moves").reshape(S, nB, W, 6)
        _MOVES[key] = (hyp, mv, _expect(oracle, *recs, bc.cfg.end_token), moves_rec, S, p, name)
    return _MOVES[key]


@pytest.mark.parametrize("form,kind,W,shape", MOVE_CASES)
def test_moves_equal_the_reference_on_the_records(rv, handles, oracle, form, kind, W, shape):
    import torch
    hyp, mv, e, rec, S, p, name = _moves_result(rv, handles, oracle, form, kind, W, shape)
    tag = f"moves {form} {name} W={W} {shape}"
    assert S == STEPS, (tag, S)
    _assert_conditions(e, name, W, tag)
    # the beam half: the expectation from the records, and the all-beams call's bytes
    _assert_equal(hyp, e, tag)
    _same_fields(hyp, _result(rv, handles, oracle, form, kind, W, shape)[0], tag + ": the beam of a moves call")
    # the six outputs: moves_reference's finalize in numpy fp32 over the call's step_moves, extended parents and lengths, bit for bit
    want = M.finalize(rec, e["par"], hyp.lengths, dtype=np.float32)
    for k in M.FIELDS:
        g = getattr(mv, k)
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, (tag, k, g.shape, g.dtype)
        assert np.array_equal(_bits(g), _bits(want[k])), (tag, k, np.argwhere(_bits(g) != _bits(want[k]))[:5].tolist())
    live = np.arange(S)[None, :, None] < hyp.lengths[:, None, :]
    assert (mv.peak[live] >= 0).all() and (mv.peak[live] < p["raw"].shape[1] + p["ev"].shape[1]).all() and (mv.peak[~live] == -1).all(), tag
    # the parent-row rule is exercised late: a hypothesis whose slot at a column >= 32 differs from the row that produced its token
    if name == "long":
        par_row = np.take_along_axis(np.transpose(e["par"], (1, 0, 2)), e["slots"], 2)
        assert (live & (par_row != e["slots"]))[:, I.HALF:].any(), (tag, "parent row == slot in every column from 32")
    # the records' ids and parents are the fp64 decode's, so the rows the reference picked are the right ones
    o = p["o"]
    assert np.array_equal(e["ids"], o["ids"]) and np.array_equal(e["par"], o["par"]), (tag, "the call left the fp64 decode")
    assert np.allclose((mv.raw_mass + mv.event_mass)[live], 1.0, atol=1e-5), (tag, "the two segments' masses do not sum to 1")
    # host, device and asynchronous forms: the same bytes
    bc = _ready(rv, handles, form, name, shape)
    x = _x("joint", p["raw"], p["ev"])
    dh, dm = bc.beam_search_moves(tuple(torch.from_numpy(a.copy()).cuda() for a in x), W, L)
    assert all(t.is_cuda for t in dh) and all(t.is_cuda for t in dm)
    ah, am = bc.collect(bc.submit_beam_search(x, W, L, moves=True))
    for what, (h2, m2) in (("device", (_np_beams(dh), _np_moves(dm))), ("asynchronous", (_np_beams(ah), _np_moves(am)))):
        _same_fields(hyp, h2, f"{tag} {what}")
        _same_fields(mv, m2, f"{tag} {what}")


# ---------------------------------------------------------------------------------------------- 5: the fused calls
@pytest.mark.parametrize("name,W", [("ragged", 1), ("long", 5), ("long", 8)])
def test_fused_calls_fill_and_compact_a_63_letter_row(rv, handles, oracle, name, W):
    p = I.passes(rv, oracle, "luong1", name, W)
    bc = _ready(rv, handles, "persistent", name)
    raw, ev = p["raw"], p["ev"]
    tag = f"calls {name} W={W}"
    entry, tok, sc, S = _beam_entry_points(bc, raw, ev, W, L=L)[0]
    assert S == STEPS and np.array_equal(tok, p["o"]["tokens"][:, :, 0]), (tag, "the best hypotheses are not the fp64 decode's")
    strings = bc.tokens_to_nuc_sequences(tok)
    assert strings == oracle.tokens_to_nuc_sequences(tok)
    host_probs = oracle.calc_prob_logits_beam_search_scores(sc)
    letters = tok >= 3
    counts = letters.sum(1)
    full = [b for b in range(6) if counts[b] == STEPS]
    assert full, (tag, "no 63-letter row", counts.tolist())
    if name == "ragged":
        _, inner = I.assert_ragged(tok, tag)
    print(f"{tag}: letters {counts.tolist()}")
    for entry, bases, lens, probs, Sc in _calls_entry_points(bc, raw, ev, W, L=L):
        t = f"{tag} {entry}"
        assert Sc == S and lens.tolist() == counts.tolist() == [len(s) for s in strings], (t, lens.tolist(), counts.tolist())
        for b in range(6):
            assert bases[b, :lens[b]].tobytes().decode("ascii") == strings[b], (t, b)
            assert (bases[b, lens[b]:] == 0).all(), (t, b, "bases beyond the chunk's letters")
        for b in full:
            assert (bases[b] != 0).all(), (t, b, "a 63-letter row with a zero")
        if name == "ragged":
            for b in inner:                    # the letters behind the non-letter id moved to the front: the tail is zero
                last = int(np.nonzero(letters[b])[0][-1])
                assert lens[b] <= last and (bases[b, :lens[b]] != 0).all() and (bases[b, lens[b]:last + 1] == 0).all(), (t, b)
        assert np.abs(probs - host_probs).max() < 1e-6, (t, "probs", float(np.abs(probs - host_probs).max()))
        _no_sentinel(lens, probs)
    bases, probs, lens = bc.collect_calls(bc.submit_calls((raw, ev), W, L))
    assert lens.tolist() == counts.tolist() and np.abs(probs - host_probs).max() < 1e-6, (tag, "submit_calls / collect_calls")


# ---------------------------------------------------------------------------------------------- 6: greedy
def test_greedy_at_the_longest_output(rv, handles, oracle):
    g = I.greedy_passes(rv, oracle)
    bc = _ready(rv, handles, "persistent", "ragged")
    V, pad_token = bc.cfg.vocab, bc.cfg.pad_token
    twin = dict(step_logits=float(np.abs(g["tlg"] - g["olg"]).max()))
    assert np.array_equal(g["tg"], g["og"]), "the twin's greedy ids leave the fp64 decode"
    for entry, tok, lg, S in _greedy_entry_points(bc, g["raw"], g["ev"], V, L=L):
        assert _decode_forms(bc) == {(PERSIST, 1, 2, 1, 3)}, (entry, sorted(_decode_forms(bc)))
        assert S == STEPS and tok.shape == (6, STEPS) and lg.shape == (6, STEPS, V), (entry, S)
        assert np.array_equal(tok, g["og"]), (entry, "ids leave the fp64 decode on rows", np.nonzero((tok != g["og"]).any(1))[0].tolist())
        err = dict(step_logits=float(np.abs(lg - g["olg"]).max()))
        _assert_twin(err, twin, f"greedy L=64 {entry}")
        assert err["step_logits"] < TOL, (entry, err)
        _no_sentinel(tok, lg)
    # three chunks whose search ends after a few steps: the columns from S to 62 of the [B, 63] buffers
    e = I.greedy_passes(rv, oracle, rows=I.GREEDY_EARLY_ROWS)
    So = e["og"].shape[1]
    for entry, tok, lg, S in _greedy_entry_points(bc, e["raw"], e["ev"], V, L=L):
        assert S == So < I.HALF and np.array_equal(tok[:, :S], e["og"]), (entry, S, So)
        assert float(np.abs(lg[:, :S] - e["olg"]).max()) < TOL, entry
        assert (tok[:, S:] == pad_token).all() and (lg[:, S:].view(np.uint32) == 0).all(), (entry, "columns beyond S")
        _no_sentinel(tok, lg)


# ---------------------------------------------------------------------------------------------- 7: members that stop early inside a long row
def _submit(bc, fn, raw, ev, W):
    t = ctypes.c_int32(-1)
    bc._check(getattr(bc._lib, fn)(bc._h, _p(raw), _p(ev), raw.shape[0], raw.shape[1], ev.shape[1], W, L, ctypes.byref(t)), fn)
    return t.value


def _collect_beam(rv, bc, ticket, nB, W):
    tok, sc, S = _filled((nB, STEPS), np.int32), _filled((nB, STEPS), np.float32), ctypes.c_int32(-1)
    bc._check(bc._lib.rv_beam_search_collect(bc._h, ticket, _p(tok), _p(sc), ctypes.byref(S)), "rv_beam_search_collect")
    return [tok, sc], S.value


def _collect_all(rv, bc, ticket, nB, W):
    bufs, S = _host_bufs(nB, W, steps=STEPS), ctypes.c_int32(-1)
    st = rv._capi.CRvBeams(*[_p(a) for a in bufs])
    bc._check(bc._lib.rv_beam_search_collect_all(bc._h, ticket, ctypes.byref(st), ctypes.byref(S)), "rv_beam_search_collect_all")
    return bufs, S.value


def _collect_moves(rv, bc, ticket, nB, W):
    bufs, mv, S = _host_bufs(nB, W, steps=STEPS), _move_bufs(nB, W, STEPS), ctypes.c_int32(-1)
    st, sm = rv._capi.CRvBeams(*[_p(a) for a in bufs]), rv._capi.CRvMoves(*[_p(a) for a in mv])
    bc._check(bc._lib.rv_beam_search_collect_moves(bc._h, ticket, ctypes.byref(st), ctypes.byref(sm), ctypes.byref(S)), "rv_beam_search_collect_moves")
    return bufs + mv, S.value


def _moves_host(rv, bc, raw, ev, W):
    bufs, mv, S = _host_bufs(raw.shape[0], W, steps=STEPS), _move_bufs(raw.shape[0], W, STEPS), ctypes.c_int32(-1)
    st, sm = rv._capi.CRvBeams(*[_p(a) for a in bufs]), rv._capi.CRvMoves(*[_p(a) for a in mv])
    bc._check(bc._lib.rv_beam_search_moves(bc._h, _p(raw), _p(ev), raw.shape[0], raw.shape[1], ev.shape[1], W, L, ctypes.byref(st), ctypes.byref(sm),
                                           ctypes.byref(S)), "rv_beam_search_moves")
    return bufs + mv, S.value


def _same_buffers(got, want, tag):
    (g, Sg), (w, Sw) = got, want
    assert Sg == Sw, (tag, "S", Sg, Sw)
    for i, (a, b_) in enumerate(zip(g, w)):
        assert a.shape == b_.shape and a.tobytes() == b_.tobytes(), (tag, "buffer", i, np.argwhere(_bits(a) != _bits(b_))[:5].tolist())
    _no_sentinel(*g)


def test_members_that_stop_early_inside_a_long_row(rv, handles, oracle):
    W = 5
    p = I.passes(rv, oracle, "luong1", "spread", W)
    bc = _ready(rv, handles, "persistent", "spread")
    raw, ev = p["raw"], p["ev"]
    early = [1, 3, 4]
    slabs = [(np.ascontiguousarray(raw[early]), np.ascontiguousarray(ev[early])), (raw, ev), (raw[:0].copy(), ev[:0].copy())]
    pad_token = bc.cfg.pad_token
    # the synchronous calls, on sentinel-filled buffers of the full width
    sync_beam, sync_all, sync_moves = [], [], []
    for r_, e_ in slabs:
        entry, tok, sc, S = _beam_entry_points(bc, r_, e_, W, L=L)[0] if r_.shape[0] else ("", _filled((0, STEPS), np.int32), _filled((0, STEPS), np.float32), 0)
        sync_beam.append(([tok, sc], S))
        sync_all.append(_all_host(rv, bc, r_, e_, W))
        sync_moves.append(_moves_host(rv, bc, r_, e_, W))
    Ss = [s for _, s in sync_beam]
    print(f"S of the three slabs: {Ss}")
    assert Ss[1] == STEPS and 2 <= Ss[0] < I.HALF and Ss[2] == 0, ("badly chosen: S of the slabs", Ss)
    assert [s for _, s in sync_all] == Ss and [s for _, s in sync_moves] == Ss
    (tok, sc), S0 = sync_beam[0]
    assert (tok[:, S0:] == pad_token).all() and (sc[:, S0:].view(np.uint32) == 0).all(), "the columns from S to 62 of the early slab"
    assert np.array_equal(tok[:, :S0], p["o"]["tokens"][early, :S0, 0]) and (p["o"]["tokens"][early, S0:, 0] == bc.cfg.end_token).all()
    for a in sync_all[0][0][:3] + sync_moves[0][0][:3]:
        assert (a[:, :S0].view(np.uint32) != 0).any() and len(set(a[:, S0:].reshape(-1).tolist())) == 1, "one fill value beyond S"

    def round_of(submit, collect, sync, tag):
        tickets = [_submit(bc, submit, r_, e_, W) for r_, e_ in slabs]
        for i, (t, (r_, _)) in enumerate(zip(tickets, slabs)):
            _same_buffers(collect(rv, bc, t, r_.shape[0], W), sync[i], f"{tag}, slab {i}")

    try:
        bc.set_async_depth(4)
        bc.set_coalesce(3)                                   # (a) one coalesced group of three
        g0, s0, _, in_force = _stats(bc)
        assert in_force == 3
        round_of("rv_beam_search_submit", _collect_beam, sync_beam, "coalesced")
        g1, s1, largest, _ = _stats(bc)
        assert (g1 - g0, s1 - s0) == (1, 3) and largest >= 3, ("the group did not form", g0, s0, g1, s1, largest)
        bc.set_coalesce(0)                                   # (b) uncoalesced
        round_of("rv_beam_search_submit", _collect_beam, sync_beam, "uncoalesced")
        assert tuple(_stats(bc)[:2]) == (g1, s1), "coalesce 0 must not form groups"
        bc.set_async_depth(3)                                # (c) the slab graph: three contexts, so that each slab meets its context again
        bc.set_option("slab_graph", 1)
        for rep in ("capture", "replay", "second replay"):
            round_of("rv_beam_search_submit", _collect_beam, sync_beam, f"slab_graph {rep}")
        bc.set_option("slab_graph", 0)
        bc.set_async_depth(4)
        round_of("rv_beam_search_submit_all", _collect_all, sync_all, "submit_all / collect_all")          # (d)
        round_of("rv_beam_search_submit_moves", _collect_moves, sync_moves, "submit_moves / collect_moves")  # (e)
    finally:
        bc.set_option("slab_graph", 0)
        bc.set_async_depth(2)
        bc.set_coalesce(-1)


# ---------------------------------------------------------------------------------------------- 8: rv_score_logits at S = 64
def test_scoring_kernel_at_64_positions(rv):
    """test_teacher_forced_gpu.test_scoring_kernel_alone's chosen logits on 64 columns: lane 63 is live and its label is not padding."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=8, max_raw_len=27, max_event_len=6, max_output_len=64)
    Vv = bc.cfg.vocab
    pad, start, end = bc.cfg.pad_token, bc.cfg.start_token, bc.cfg.end_token
    rng = np.random.default_rng(5 + Vv)
    nB, S = 6, 64
    lg = (rng.standard_normal((nB, S, Vv)) * 3).astype(np.float32)
    lab = rng.integers(0, Vv, size=(nB, S)).astype(np.int32)
    lg[0, 0] = 0.25
    lg[0, 1, :] = -1.0; lg[0, 1, Vv - 1] = 2.0; lg[0, 1, Vv // 2] = 2.0
    lg[0, 2] = 80.0 * np.where(np.arange(Vv) % 2, -1.0, 1.0)
    lab[0, 2] = 1
    lg[0, 3] = -80.0; lg[0, 3, Vv - 1] = 80.0
    lab[1] = pad
    lg[2] = 0.0
    lab[[0, 2, 3, 4, 5], 63] = [3, 4, 5, 6, end]              # column 63: a label that is not padding, in every row but the padding row
    lg[3, 63] = lg[0, 1]                                     # ... a tie and a large magnitude in the last lane too
    lg[4, 63] = lg[0, 2]
    score = lambda lg_, lab_, omit: (lambda r: type(r)(*[a.numpy() for a in r]))(bc.score_logits(lab_, lg_, omit))
    for omit in ((pad, start, end), (start, end), ()):
        r = score(lg, lab, omit)
        assert np.array_equal(r.sample_id, np.argmax(lg, -1)), "argmax, first maximum on ties"
        assert r.sample_id[0, 1] == Vv // 2 and r.sample_id[0, 0] == 0 and r.sample_id[3, 63] == Vv // 2
        n_match, n_counted = np_counts(lab, r.sample_id, omit)
        assert np.array_equal(r.n_match, n_match) and np.array_equal(r.n_counted, n_counted), omit
        assert np.array_equal(r.n_labels, (lab != pad).sum(-1)) and r.n_labels[1] == 0
    assert np.isfinite(r.nll).all() and (r.nll[:, 63][lab[:, 63] != pad] > 0).all()
    assert (r.nll[lab == pad] == 0).all() and r.nll_sum[1] == 0
    ref = np_nll(lg.astype(np.float64), lab, pad)
    f32 = np_nll(lg, lab, pad)
    assert f32.dtype == np.float32
    e_gpu, e_np = float(np.abs(r.nll - ref).max()), float(np.abs(f32 - ref).max())
    e63 = float(np.abs(r.nll[:, 63] - ref[:, 63]).max())
    print(f"score kernel S=64: max |nll - fp64| gpu {e_gpu:.2e} (column 63: {e63:.2e}), numpy float32 {e_np:.2e}")
    assert e_gpu <= 2 * e_np + 1e-6, (e_gpu, e_np)
    want = np.zeros(nB, np.float32)
    for s in range(S):
        want = want + r.nll[:, s]
    assert np.array_equal(r.nll_sum, want), "nll_sum is not the in-order fp32 sum of 64 terms"
    with pytest.raises(rv._capi.RavventHipError, match=r"RV_EINVAL: S=65 outside \[0,64\]"):
        score(np.zeros((nB, 65, Vv), np.float32), np.zeros((nB, 65), np.int32), ())
    bc.close()


# ---------------------------------------------------------------------------------------------- 9: the short end
@pytest.mark.parametrize("form", ["persistent", "per_step_graph"])
@pytest.mark.parametrize("name", ["long", "spread"])
def test_a_single_step(rv, handles, oracle, form, name):
    """L = 2 on the handles of 64: one step, one column, lane 0 alone."""
    W = 5
    p = I.passes(rv, oracle, "luong1", name, W)
    bc = _ready(rv, handles, form, name)
    x = _x("joint", p["raw"], p["ev"])
    tag = f"L=2 {form} {name}"
    got = _np_beams(bc.beam_search_hypotheses(x, W, 2))
    _assert_form(rv, bc, form, W, "A", tag)
    assert got.tokens.shape == (6, 1, W), (tag, got.tokens.shape)
    e = _expect(oracle, *_records(bc, 1, 6, W, FORMS[form][2] is not None), bc.cfg.end_token)
    _assert_equal(got, e, tag)
    o = p["o"]
    assert np.array_equal(e["ids"][0], o["ids"][0]) and np.array_equal(e["par"][0], o["par"][0]), (tag, "the step left the fp64 decode")
    assert I.max_error(got.log_probs, o["sc"][0]) < TOL and np.array_equal(got.lengths, np.ones((6, W), np.int32)), tag
    hyp, mv = bc.beam_search_moves(x, W, 2)
    hyp, mv = _np_beams(hyp), _np_moves(mv)
    _same_fields(hyp, got, tag + ": the beam of a moves call")
    rec = bc.get_tensor("step_moves").reshape(1, 6, W, 6)
    want = M.finalize(rec, e["par"], hyp.lengths, dtype=np.float32)
    for k in M.FIELDS:
        assert getattr(mv, k).shape == (6, 1, W) and np.array_equal(_bits(getattr(mv, k)), _bits(want[k])), (tag, k)
    assert (mv.peak >= 0).all(), tag


@pytest.mark.parametrize("form,W", [("persistent", 5), ("persistent", 8), ("bahdanau", 5), ("two_cells", 5), ("per_step_graph", 8)])
def test_a_one_token_hypothesis_in_a_63_column_row(rv, handles, oracle, form, W):
    """On "spread" hypothesis 0 ends at its first step: end_token in every column of its row and one path score repeated 63 times,
    beside hypotheses that run to the last column."""
    got, e, S, p, name = _result(rv, handles, oracle, form, "spread", W)
    one = [b for b in range(6) if got.lengths[b, 0] == 1]
    assert one and S == STEPS, (form, W, "no hypothesis 0 of length 1", got.lengths[:, 0].tolist())
    for b in one:
        assert (got.tokens[b, :, 0] == p["cfg"].end_token).all(), (form, W, b, got.tokens[b, :, 0].tolist())
        assert (got.path_scores[b, :, 0].view(np.uint32) == got.path_scores[b, 0, 0].view(np.uint32)).all(), (form, W, b, "path score")
        assert got.path_scores[b, 0, 0].view(np.uint32) == got.log_probs[b, 0].view(np.uint32), (form, W, b)
    assert any(got.lengths[b].max() == STEPS for b in one), "no chunk holds a one-token hypothesis beside a 63-token one"
