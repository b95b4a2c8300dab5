"""The moves (rv_beam_search_moves*, Basecaller.beam_search_moves): where in the chunk's signal each token of each hypothesis lies.

Two kernels stand behind a moves call, and each is held to what it reads.  The decode reduces the alignments of every step to one
record per beam row (DecState::step_moves): test_records_are_the_forms_own_alignments makes the call with the form's alignment tap on
and recomputes the sums in fp64 from the fp32 alignments the tap stored -- the values the context product consumed.
k_dec_finalize_moves is a pure function of the records the decode leaves: test_finalize_is_a_function_of_the_records rebuilds its
six outputs from the GPU's own step_moves / parent_ids / step_ids / chunk_steps with test_beams_gpu._expect's slots and numpy's fp32
division, bit for bit, fills included.  test_the_beam_is_untouched holds the beam outputs of a moves call to the bytes of the
existing calls, test_against_fp64 holds the outputs to the fp64 oracle through tests/moves_reference.py, test_contract covers the
entry points.  On the per-step decode a tapped call takes the launches of an untapped one (up to beam 5 the two-pass kernel leaves the
records beside the single-pass attend, and the tap is that kernel's); test_untapped_per_step_call_is_the_tapped_one holds the call
without taps to the tapped one's bits.

Shapes (B = 6 chunks of test_kernel_forms_gpu._slab):
  A      joint 40 + 8, L = 14: the beams tests' own shape, with their seeds (test_beams_gpu.SEEDS) and end-token bias.
  B      joint 61 + 9, T_m = 70, L = 10: the low edge of the NIT 8 band of k_dec_persist; the segment split at t = 61 falls inside a
         k-block of 8 steps and inside a 32-row group.  Braw: raw only, T_r = 70.  Bev: event only, T_e = 33.
  C      joint 308 + 44, T_m = 352, L = 6: the upper edge of the NIT 11 band.
Seeds of B, Braw, Bev and C, searched on the CPU as test_beams_gpu's docstring describes (weight seed 1, gain 1.5, end-token bias
-0.02, slab seeds 1, 2, .. in turn, beam 5, Luong with one cell): at slab seed 1, the first tried, the oracle's numpy fp32 twin
returns the fp64 pass's step ids and parents on all six chunks of every one of the four shapes, and the fp64 records are not vacuous
in the sense of test_beams_gpu._assert_not_vacuous (on all six chunks and on chunks 0 .. 4); the steps at which the chunks' beams are
all finished: B [9, 7, 9, 4, 8, 9] (S = 9), Braw [4, 5, 5, 4, 9, 7], Bev [9, 9, 9, 4, 9, 9], C [4, 5, 5, 4, 5, 4] (S = 5).  The tests
assert non-vacuity on the GPU's own records before they rely on a slab.
  D      joint splits with the raw / event boundary where the per-segment reductions can go wrong (s_movesTr, persist_moves_arg:
         DESIGN.md section 12): one raw sample (1 + 63, 1 + 351), one event (351 + 1), the boundary exactly on a 32-row group edge
         (32 + 33, 64 + 192), and T_e >= T_r at the full 352 steps (176 + 176); L = 10 up to T_m = 256, L = 6 at 352.  The D shapes share
         one handle per (attention, cells), sized for any split of 352 steps.
Seeds of D (BOUNDARY_SEEDS), by the same search: the first slab seeds at which the twin returns the fp64 ids and parents on all six
chunks and the fp64 records are not vacuous on all six and on chunks 0 .. 4 are 1, 2, 1, 3, 1, 2 in the order of SHAPES (the lower
seeds fail only because their chunks finish together); the chunks' beams are all finished at 1 + 63 [9, 9, 7, 9, 9, 5], 32 + 33
[5, 9, 5, 9, 6, 4], 64 + 192 [6, 9, 9, 9, 9, 9], 1 + 351 [5, 5, 4, 5, 5, 5], 351 + 1 [4, 5, 5, 5, 5, 5], 176 + 176 [5, 3, 5, 5, 5, 5].
test_against_fp64 counts its witnesses of non-vacuity (a parent row whose position differs from the slot's by more than four times
the tolerance) in the longer segment of a shape: with one raw sample every raw position is 0."""
import ctypes

import numpy as np
import pytest

import moves_reference as M
from test_beams_gpu import (END_BIAS, FORMS, SEEDS, SPLIT_SEEDS, SPLIT_SHAPE, _assert_not_vacuous, _bits, _expect, _np_beams, _records,
                            _stats)
from test_config_space_gpu import _filled, _no_sentinel
from test_kernel_forms_gpu import ATTEND, B, FLASH, PERSIST, _decode_forms, _handle, _set, _slab, _x
from test_parity_gpu import _near_tie_gap

pytestmark = pytest.mark.gpu

SHAPES = {"A": ("joint", 40, 8, 14), "B": ("joint", 61, 9, 10), "Braw": ("raw", 70, 0, 10), "Bev": ("event", 0, 33, 10),
          "C": ("joint", 308, 44, 6),
          "D1+63": ("joint", 1, 63, 10), "D32+33": ("joint", 32, 33, 10), "D64+192": ("joint", 64, 192, 10),
          "D1+351": ("joint", 1, 351, 6), "D351+1": ("joint", 351, 1, 6), "D176+176": ("joint", 176, 176, 6)}
NIT = {48: 2, 70: 8, 33: 2, 352: 11, 64: 2, 65: 8, 256: 8}          # the k_dec_persist band that serves T_m
OTHER_SEEDS = (1, 1)                          # (weight seed, slab seed) of B, Braw, Bev, C: see the module docstring
BOUNDARY_SEEDS = {"D1+63": 1, "D32+33": 2, "D64+192": 1, "D1+351": 3, "D351+1": 1, "D176+176": 2}     # slab seeds of the D shapes
MX = dict(matrix_attention=1, matrix_cell=1)
PERSIST_OPTS = dict(persistent_decode=1, use_graph=1, decode_split=1)
# form -> (attention, decoder cells, options, the ATT of k_dec_persist it must run or None for the per-step kernels, beam widths on A)
MOVE_FORMS = {name: (a, D, {**opts, **MX}, att, ws) for name, (a, D, opts, att, ws) in FORMS.items()}
MOVE_FORMS.update({
    "att0": ("luong", 1, dict(PERSIST_OPTS, matrix_attention=0, matrix_cell=0), 0, (1, 3, 5, 8)),
    "att1": ("bahdanau", 1, dict(PERSIST_OPTS, matrix_attention=1, matrix_cell=0), 1, (1, 3, 5, 8)),
    "att2": ("luong", 1, dict(PERSIST_OPTS, matrix_attention=1, matrix_cell=0), 2, (1, 3, 5, 8)),
})
CASES = [(f, W, "A") for f, spec in MOVE_FORMS.items() for W in spec[4]] + \
        [(f, 5, sh) for sh in ("B", "Braw", "Bev", "C", *BOUNDARY_SEEDS) for f in MOVE_FORMS]
FIELDS = M.FIELDS


# ---------------------------------------------------------------------------------------------- handles and slabs: made once
_HANDLES, _BASECALLERS = {}, {}


@pytest.fixture(scope="module")
def handles(rv):
    def get(shape, attention, D):
        key = (shape, attention, D)
        if key not in _HANDLES:
            mode, TR, TE, L = SHAPES[shape]
            wseed, sseed = SEEDS[(attention, D)] if shape == "A" else (OTHER_SEEDS[0], BOUNDARY_SEEDS.get(shape, OTHER_SEEDS[1]))
            # the D shapes share one handle per (attention, cells): the same weights, room for every split of 352 steps
            hkey, TRm, TEm, Lm = (("D", attention, D), 351, 351, 10) if shape in BOUNDARY_SEEDS else (key, max(TR, 1), max(TE, 1), L)
            if hkey not in _BASECALLERS:
                _BASECALLERS[hkey] = _handle(rv, mode, attention, D, wseed, Tr_max=TRm, Te_max=TEm, L=Lm, end_bias=END_BIAS)
            bc, w = _BASECALLERS[hkey]
            raw, ev = _slab(mode, TR, TE, seed=sseed)
            praw, pev = raw.copy(), ev.copy()
            praw[5], pev[5] = 0.0, 0.0                # the same slab with its last chunk padding from end to end
            for a in (raw, ev, praw, pev):
                a.setflags(write=False)
            _HANDLES[key] = (bc, w, (raw, ev), (praw, pev))
        return _HANDLES[key]
    yield get
    for bc, _ in _BASECALLERS.values():
        bc.close()
    _HANDLES.clear()
    _BASECALLERS.clear()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _beam_bufs(nB, W, steps):
    return [_filled((nB, steps, W), np.int32), _filled((nB, steps, W), np.float32), _filled((nB, steps, W), np.float32),
            _filled((nB, W), np.float32), _filled((nB, W), np.int32)]


def _move_bufs(nB, W, steps):
    return [_filled((nB, steps, W), np.int32 if k == "peak" else np.float32) for k in FIELDS]


def _raw_call(rv, bc, shape, raw, ev, W, L=None, beams=None, moves=None):
    """rv_beam_search_moves on pre-filled host buffers of the full width L - 1 -> (rc, S, beam buffers, move buffers)."""
    mode, TR, TE, Ls = SHAPES[shape]
    L = Ls if L is None else L
    nB = raw.shape[0]
    beams = _beam_bufs(nB, W, L - 1) if beams is None else beams
    moves = _move_bufs(nB, W, L - 1) if moves is None else moves
    S = ctypes.c_int32(-1)
    sb = rv._capi.CRvBeams(*[_p(a) for a in beams])
    sm = rv._capi.CRvMoves(*[_p(a) for a in moves])
    rc = bc._lib.rv_beam_search_moves(bc._h, _p(raw) if mode != "event" else None, _p(ev) if mode != "raw" else None, nB, TR, TE, W, L,
                                      ctypes.byref(sb), ctypes.byref(sm), ctypes.byref(S))
    return rc, S.value, beams, moves


def _np_moves(mv):
    return type(mv)(*[a.cpu().numpy().copy() for a in mv])


def _tapped_call(bc, x, W, L, Tm, persist):
    """One moves call with the form's alignment tap on -> (hypotheses, moves, S, step_moves, alignments, ids, parents, chunk steps)."""
    tap = "persist_taps" if persist else "debug_taps"
    bc.set_option(tap, 1)
    try:
        hyp, mv = bc.beam_search_moves(x, W, L)
        hyp, mv = _np_beams(hyp), _np_moves(mv)
        S = hyp.tokens.shape[1]
        nB = hyp.tokens.shape[0]
        forms = _decode_forms(bc)
        ids, par, sc, cs = _records(bc, S, nB, W, persist)
        rec = bc.get_tensor("step_moves").reshape(S, nB, W, 6)
        al = bc.get_tensor("step_alignments").reshape(S, nB, W, Tm)
    finally:
        bc.set_option(tap, 0)
    return dict(hyp=hyp, mv=mv, S=S, rec=rec, al=al, ids=ids, par=par, sc=sc, cs=cs, forms=forms)


def _assert_form(forms, W, Tm, D, att, tag, aside=None):
    """aside (per-step forms): True = the single-pass attend ran the steps and the two-pass kernel left the records beside it (Luong,
    beam <= 5: the default of that path), False = the two-pass kernel alone, None = not looked at."""
    if att is None:
        assert not any(r[0] == PERSIST for r in forms), (tag, sorted(forms))
        if aside is not None:
            kinds = {r[0] for r in forms}
            assert kinds == ({FLASH, ATTEND} if aside else {ATTEND}), (tag, "attend kernels", sorted(forms))
    else:
        assert {r for r in forms if r[0] == PERSIST} == {(PERSIST, W, NIT[Tm], D, att)}, (tag, sorted(forms))


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("form,W,shape", CASES)
def test_records_are_the_forms_own_alignments(handles, form, W, shape):
    attention, D, opts, att, _ = MOVE_FORMS[form]
    mode, TR, TE, L = SHAPES[shape]
    Tm, Tsplit = TR + TE, (TR if mode != "event" else 0)
    bc, _, slab, padded = handles(shape, attention, D)
    _set(bc, opts)
    tag = f"{form} W={W} {shape}"
    r = _tapped_call(bc, _x(mode, *slab), W, L, Tm, att is not None)
    # (with the tap on a per-step call keeps its route: up to beam 5 the records are the two-pass launch's beside the single-pass attend)
    _assert_form(r["forms"], W, Tm, D, att, tag, aside=W <= 5)
    rel = (Tm + 2) * 2.0 ** -23

    def check(r, chunks):
        worst = 0.0
        for b in chunks:
            n = int(r["cs"][b])
            al, rec = r["al"][:n, b], r["rec"][:n, b].astype(np.float64)
            assert not np.isnan(al).any(), (tag, b, "a tapped alignment is NaN")
            ref = M.records(al, Tsplit)
            for c in range(4):
                zero = ref[..., c] == 0
                assert (rec[..., c][zero] == 0).all(), (tag, b, c, "a sum that must be exactly 0")
                err = np.abs(rec[..., c] - ref[..., c])[~zero] / ref[..., c][~zero]
                if err.size:
                    worst = max(worst, float(err.max()))
                    assert err.max() <= rel, (tag, b, c, float(err.max()), rel)
            pk = al.argmax(-1)                                                        # the first maximum of the fp32 alignments
            assert (r["rec"][:n, b, :, 5] == pk).all(), (tag, b, "peak_t", r["rec"][:n, b, :, 5].tolist(), pk.tolist())
            assert np.array_equal(_bits(r["rec"][:n, b, :, 4]), _bits(np.take_along_axis(al, pk[..., None], -1)[..., 0])), (tag, b, "peak_weight")
        return worst

    worst = check(r, range(B))
    print(f"{tag}: S = {r['S']}, chunk steps {r['cs'].tolist()}, max relative error of the sums {worst:.2e} (bound {rel:.2e})")
    # the slab whose last chunk is padding from end to end
    q = _tapped_call(bc, _x(mode, *padded), W, L, Tm, att is not None)
    n5 = int(q["cs"][5])
    assert n5 > 0 and np.isnan(q["rec"][:n5, 5, :, :5]).all() and (q["rec"][:n5, 5, :, 5] == -1).all(), (tag, "the padding chunk's records")
    for b in range(5):
        n = min(int(r["cs"][b]), int(q["cs"][b]))
        assert n > 0 and np.array_equal(_bits(r["rec"][:n, b]), _bits(q["rec"][:n, b])), (tag, b, "records depend on the slab")
    check(q, range(5))


# ---------------------------------------------------------------------------------------------- 2
def _expect_moves(rec, e, lengths):
    """The six outputs [B,S,W] from fp32 records [S,B,W,6] with _expect's extended parents and slots: numpy fp32 division."""
    S, nB, W = e["par"].shape
    f32 = np.float32
    out = dict(raw_pos=np.full((nB, S, W), -1, f32), raw_mass=np.zeros((nB, S, W), f32), event_pos=np.full((nB, S, W), -1, f32),
               event_mass=np.zeros((nB, S, W), f32), peak=np.full((nB, S, W), -1, np.int32), peak_weight=np.zeros((nB, S, W), f32))
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(nB):
            for w in range(W):
                for t in range(min(S, int(lengths[b, w]))):
                    m = rec[t, b, e["par"][t, b, e["slots"][b, t, w]]].astype(f32)
                    out["raw_mass"][b, t, w], out["event_mass"][b, t, w], out["peak_weight"][b, t, w] = m[0], m[2], m[4]
                    out["raw_pos"][b, t, w] = f32(-1) if m[0] == 0 else m[1] / m[0]
                    out["event_pos"][b, t, w] = f32(-1) if m[2] == 0 else m[3] / m[2]
                    out["peak"][b, t, w] = int(m[5])
    return out


@pytest.mark.parametrize("form", ["persistent", "per_step_graph"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_finalize_is_a_function_of_the_records(rv, handles, oracle, form, shape):
    attention, D, opts, att, _ = MOVE_FORMS[form]
    mode, TR, TE, L = SHAPES[shape]
    W, steps = 5, L - 1
    bc, _, (raw, ev), (praw, pev) = handles(shape, attention, D)
    _set(bc, opts)
    for kind, (r_, e_) in (("slab", (raw, ev)), ("with a padding chunk", (praw, pev))):
        tag = f"{form} {shape} {kind}"
        rc, S, beams, moves = _raw_call(rv, bc, shape, r_, e_, W)
        bc._check(rc, "rv_beam_search_moves")
        _assert_form(_decode_forms(bc), W, TR + TE, D, att, tag)
        e = _expect(oracle, *_records(bc, S, B, W, att is not None), bc.cfg.end_token)
        _assert_not_vacuous(e, W, tag, rows=slice(None) if kind == "slab" else slice(0, 5))
        rec = bc.get_tensor("step_moves").reshape(S, B, W, 6)
        assert np.array_equal(beams[4], e["lengths"]), (tag, "lengths")
        want = _expect_moves(rec, e, beams[4])
        if kind != "slab":
            own = np.arange(S)[:, None] < beams[4][5][None, :]          # the columns its hypotheses own
            assert S == steps and own.any() and np.isnan(want["raw_mass"][5][own]).all() and (want["peak"][5] == -1).all(), \
                (tag, "the padding chunk is not one")
        for k, got in zip(FIELDS, moves):
            fill = -1 if k in ("raw_pos", "event_pos", "peak") else 0
            full = np.full((B, steps, W), fill, got.dtype)
            full[:, :S] = want[k]
            assert np.array_equal(_bits(got), _bits(full)), (tag, k, np.argwhere(_bits(got) != _bits(full))[:5].tolist())
        _no_sentinel(*beams, *moves)
        live = np.arange(S)[None, :, None] < beams[4][:, None, :]
        assert (moves[4][:, :S][live & ~np.isnan(moves[1][:, :S])] >= 0).all(), (tag, "a live column without a peak")


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("form,W", [(f, W) for f, spec in MOVE_FORMS.items() for W in spec[4]])
def test_the_beam_is_untouched(handles, form, W):
    attention, D, opts, att, _ = MOVE_FORMS[form]
    mode, TR, TE, L = SHAPES["A"]
    bc, _, slab, padded = handles("A", attention, D)
    _set(bc, opts)
    for kind, (raw, ev) in (("slab", slab), ("with a padding chunk", padded)):
        x = _x(mode, raw, ev)
        tag = f"{form} W={W} {kind}"
        tok, sc = bc.beam_search_prediction(x, W, L)
        tok, sc = tok.numpy().copy(), sc.numpy().copy()
        all_ = _np_beams(bc.beam_search_hypotheses(x, W, L))
        hyp, mv = bc.beam_search_moves(x, W, L)
        hyp = _np_beams(hyp)
        _assert_form(_decode_forms(bc), W, TR + TE, D, att, tag)
        for k in all_._fields:
            assert getattr(hyp, k).shape == getattr(all_, k).shape and getattr(hyp, k).tobytes() == getattr(all_, k).tobytes(), (tag, k)
        assert hyp.tokens[:, :, 0].tobytes() == tok.tobytes() and np.ascontiguousarray(hyp.scores[:, :, 0]).tobytes() == sc.tobytes(), tag
        assert all(tuple(a.shape) == hyp.tokens.shape for a in mv), tag


# ---------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("form,shape", [pytest.param(f, sh, id=f if sh == "A" else f"{f}-{sh}")
                                        for sh in ("A", *BOUNDARY_SEEDS) for f in ("persistent", "per_step_graph")])
def test_against_fp64(handles, oracle, form, shape):
    W = 5
    attention, D, opts, att, _ = MOVE_FORMS[form]
    assert (attention, D) == ("luong", 1)
    mode, TR, TE, L = SHAPES[shape]
    Tm = TR + TE
    bc, w, (raw, ev), _ = handles(shape, attention, D)
    _set(bc, opts)
    r = _tapped_call(bc, _x(mode, raw, ev), W, L, Tm, att is not None)
    form = form if shape == "A" else f"{form} {shape}"
    _assert_form(r["forms"], W, Tm, D, att, form, aside=True)      # per_step_graph: the records of the default per-step route
    wseg = "raw" if TR >= TE else "event"                          # the witnesses of non-vacuity: positions in the longer segment
    wcol = 0 if wseg == "raw" else 2
    end = bc.cfg.end_token
    taps = {}
    oracle.beam_search(w, bc.cfg.oracle_cfg(), raw, ev, W, L, dtype=np.float64, taps=taps)
    oids, opar, oln, a64 = taps["step_ids"], taps["parent_ids"], taps["lengths"], taps["step_alignments"]
    So = oids.shape[0]
    ref = M.moves_reference(a64, oids, opar, oln, TR, end)
    rec64 = M.records(a64, TR)
    slot, _ = M.slots(opar, oln)
    left = []
    for b in range(B):
        m = min(int(r["cs"][b]), So)
        if (r["ids"][:m, b] != oids[:m, b]).any() or (r["par"][:m, b] != opar[:m, b]).any():
            gap = _near_tie_gap(oracle, taps["step_logits"][:, b], W, end)
            assert gap < 1e-4, (form, b, "left the fp64 decode with no near-tie", gap)
            left.append(b)
    assert len(left) <= 1, (form, "chunks that left the fp64 decode", left)
    if not left:
        assert r["S"] == So, (form, r["S"], So)
    mv, u = r["mv"], 2.0 ** -24
    worst_d, witnesses, tried = 0.0, 0, 0
    for b in (b for b in range(B) if b not in left):
        assert (r["hyp"].lengths[b] == oln[b]).all(), (form, b, "lengths")
        for k in range(W):
            for t in range(min(r["S"], So, int(oln[b, k]))):
                row = int(opar[t, b, slot[b, t, k]])
                d = float(np.abs(r["al"][t, b, row].astype(np.float64) - a64[t, b, row]).max())
                worst_d = max(worst_d, d)
                assert d <= 1e-4, (form, b, k, t, "alignments", d)
                tag = (form, b, k, t)
                tol_pos = {}
                for seg, n in (("raw", TR), ("event", TE)):
                    m64, p64 = ref[seg + "_mass"][b, t, k], ref[seg + "_pos"][b, t, k]
                    mg, pg = float(getattr(mv, seg + "_mass")[b, t, k]), float(getattr(mv, seg + "_pos")[b, t, k])
                    if m64 == 0:
                        assert mg == 0 and pg == -1 and p64 == -1, (tag, seg, "an exactly zero mass")
                        continue
                    assert mg != 0, (tag, seg, "a mass that is not zero")
                    assert abs(mg - m64) <= n * d + (Tm + 2) * 2 * u, (tag, seg, "mass", mg, m64, d)
                    tol_pos[seg] = n * n * d / (2 * m64) + 2 * (Tm + 2) * u * p64
                    assert abs(pg - p64) <= tol_pos[seg], (tag, seg, "pos", pg, p64, tol_pos[seg], d)
                pk = int(mv.peak[b, t, k])
                assert 0 <= pk < Tm and a64[t, b, row, pk] >= a64[t, b, row].max() - 2 * d, (tag, "peak", pk)
                # non-vacuity: the parent row is not the slot, and the two rows' fp64 positions are told apart by the tolerance
                s_ = int(slot[b, t, k])
                if row != s_ and wseg in tol_pos and rec64[t, b, s_, wcol] > 0:
                    tried += 1
                    other = rec64[t, b, s_, wcol + 1] / rec64[t, b, s_, wcol]
                    witnesses += abs(other - ref[wseg + "_pos"][b, t, k]) > 4 * tol_pos[wseg]
    print(f"{form}: S = {r['S']} (fp64 {So}), left {left}, max |alpha - fp64| = {worst_d:.2e}, parent != slot cases {tried}, of which "
          f"the rows differ by more than 4 x tolerance: {witnesses}")
    assert witnesses > 0, (form, "no case tells the parent row from the slot", tried)


# ---------------------------------------------------------------------------------------------- 4b
@pytest.mark.parametrize("shape,W", [("A", 3), ("A", 5), ("A", 8), ("B", 5), ("C", 5)])
@pytest.mark.parametrize("form", ["per_step", "per_step_graph"])
def test_untapped_per_step_call_is_the_tapped_one(rv, handles, oracle, form, shape, W):
    """The records of tests 1 and 4 come from calls with debug_taps on.  The call a user makes has it off: the same launches (the
    two-pass kernel beside the single-pass attend up to beam 5, alone above), no tap stores.  Its beam, its six outputs and -- up to
    the step at which a chunk's beams are all finished, from where the untapped single-pass kernel skips the chunk's cell output and
    nothing of it is handed out -- its records are the tapped call's bit for bit, so what those tests hold, holds for it."""
    attention, D, opts, att, _ = MOVE_FORMS[form]
    mode, TR, TE, L = SHAPES[shape]
    bc, _, (raw, ev), _ = handles(shape, attention, D)
    _set(bc, opts)
    tag = f"{form} {shape} W={W}"
    t = _tapped_call(bc, _x(mode, raw, ev), W, L, TR + TE, False)
    rc, S, beams, moves = _raw_call(rv, bc, shape, raw, ev, W)
    bc._check(rc, "rv_beam_search_moves")
    forms = _decode_forms(bc)
    _assert_form(forms, W, TR + TE, D, att, tag, aside=W <= 5)
    assert forms == t["forms"], (tag, "the tap changed the launches", sorted(forms), sorted(t["forms"]))
    assert S == t["S"], (tag, S, t["S"])
    rec = bc.get_tensor("step_moves").reshape(S, B, W, 6)
    e = _expect(oracle, *_records(bc, S, B, W, False), bc.cfg.end_token)
    _assert_not_vacuous(e, W, tag)
    for k, a in zip(t["hyp"]._fields, beams):
        a = a[:, :S] if a.ndim == 3 else a
        assert np.array_equal(_bits(a), _bits(getattr(t["hyp"], k))), (tag, "beam", k)
    for k, a in zip(FIELDS, moves):
        assert np.array_equal(_bits(a[:, :S]), _bits(getattr(t["mv"], k))), (tag, k)
    for b in range(B):
        n = int(e["fin_at"][b])
        assert n > 0 and np.array_equal(_bits(rec[:n, b]), _bits(t["rec"][:n, b])), (tag, b, "records")


# ---------------------------------------------------------------------------------------------- 5
def test_contract(rv, handles, oracle):
    import torch
    mode, TR, TE, L = SHAPES["A"]
    W, steps = 5, L - 1
    bc, _, (raw, ev), (praw, pev) = handles("A", "luong", 1)
    err = rv._capi.RavventHipError
    for opts in (MOVE_FORMS["persistent"][2], MOVE_FORMS["per_step_graph"][2]):
        _set(bc, opts)
        x = _x(mode, raw, ev)
        hyp, mv = bc.beam_search_moves(x, W, L)
        hyp, mv = _np_beams(hyp), _np_moves(mv)
        S = hyp.tokens.shape[1]
        # device inputs and outputs, and the asynchronous call: the same bytes
        dev = tuple(torch.from_numpy(a.copy()).cuda() for a in x)
        dh, dm = bc.beam_search_moves(dev, W, L)
        assert all(t.is_cuda for t in dh) and all(t.is_cuda for t in dm)
        ah, am = bc.collect(bc.submit_beam_search(x, W, L, moves=True))
        for tag, (h2, m2) in (("device", (_np_beams(dh), _np_moves(dm))), ("asynchronous", (_np_beams(ah), _np_moves(am)))):
            for k in hyp._fields:
                assert getattr(h2, k).shape == getattr(hyp, k).shape and getattr(h2, k).tobytes() == getattr(hyp, k).tobytes(), (opts, tag, k)
            for k in mv._fields:
                assert getattr(m2, k).shape == getattr(mv, k).shape and getattr(m2, k).tobytes() == getattr(mv, k).tobytes(), (opts, tag, k)
        # each member NULL in turn; all NULL
        rc, S0, beams, full = _raw_call(rv, bc, "A", raw, ev, W)
        bc._check(rc, "rv_beam_search_moves")
        assert S0 == S
        for i in range(6):
            part = _move_bufs(B, W, steps)
            part[i] = None
            rc, S1, b1, _ = _raw_call(rv, bc, "A", raw, ev, W, moves=part)
            bc._check(rc, "rv_beam_search_moves")
            assert S1 == S and all(a is None or a.tobytes() == f.tobytes() for a, f in zip(part, full)), (opts, "NULL member", i)
            assert all(a.tobytes() == f.tobytes() for a, f in zip(b1, beams)), (opts, "NULL member", i, "beams")
        rc, _, _, _ = _raw_call(rv, bc, "A", raw, ev, W, moves=[None] * 6)
        assert rc == -1 and b"null output pointer" in bc._lib.rv_last_error(bc._h), "RV_EINVAL expected"
        dpart = [None if i == 2 else torch.full((B, steps, W), 0x7F7F7F7F, dtype=torch.int32, device="cuda") for i in range(6)]
        dbeams = [torch.full(a.shape, 0x7F7F7F7F, dtype=torch.int32, device="cuda") for a in beams]
        dp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        Sv = ctypes.c_int32(-1)
        sb, sm = rv._capi.CRvBeams(*[dp(t) for t in dbeams]), rv._capi.CRvMoves(*[dp(t) for t in dpart])
        bc._check(bc._lib.rv_beam_search_moves_dev(bc._h, dp(dev[0]), dp(dev[1]), B, TR, TE, W, L, ctypes.byref(sb), ctypes.byref(sm),
                                                   ctypes.byref(Sv)), "rv_beam_search_moves_dev")
        assert Sv.value == S and all(t is None or t.cpu().numpy().tobytes() == f.tobytes() for t, f in zip(dpart, full)), (opts, "device, NULL member")
        assert all(t.cpu().numpy().tobytes() == f.tobytes() for t, f in zip(dbeams, beams)), (opts, "device beams")
    _set(bc, MOVE_FORMS["persistent"][2])
    # nothing to launch
    h0, m0 = bc.beam_search_moves(_x(mode, raw[:0], ev[:0]), W, L)
    assert h0.tokens.shape == (0, 0, W) and all(tuple(a.shape) == (0, 0, W) for a in m0)
    h1, m1 = bc.beam_search_moves(_x(mode, raw, ev), W, 1)
    assert h1.tokens.shape == (B, 0, W) and all(tuple(a.shape) == (B, 0, W) for a in m1) and (h1.lengths.numpy() == 0).all()
    # a beam wider than the handle's: the message of rv_beam_search
    narrow = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=B, max_raw_len=TR, max_event_len=TE,
                           max_output_len=L, max_beam=3)
    narrow.init_random_weights(seed=1)
    with pytest.raises(err, match=r"RV_EINVAL: beam width 5 outside \[1,3\]"):
        narrow.beam_search_moves(_x(mode, raw, ev), 5, L)
    narrow.close()
    # a moves ticket between ordinary coalesced tickets
    xs = {"a": _x(mode, raw, ev), "b": _x(mode, praw, pev)}
    sync = {k: tuple(t.numpy().copy() for t in bc.beam_search_prediction(xs[k], W, L)) for k in xs}
    wh, wm = bc.beam_search_moves(xs["b"], W, L)
    wh, wm = _np_beams(wh), _np_moves(wm)
    bc.set_async_depth(4)
    bc.set_coalesce(2)
    try:
        g0, s0, _, in_force = _stats(bc)
        assert in_force == 2
        t1 = bc.submit_beam_search(xs["a"], W, L)                  # ordinary: a group of two ...
        t2 = bc.submit_beam_search(xs["b"], W, L)                  # ... which launches full
        t3 = bc.submit_beam_search(xs["b"], W, L, moves=True)      # the moves: a slab context of its own
        t4 = bc.submit_beam_search(xs["a"], W, L)                  # ordinary: opens a group that never fills
        with pytest.raises(err, match="RV_EINVAL"):                # the wrong collect leaves the ticket in flight
            bc.collect(dict(t3, kind="all_host"))
        r3 = bc.collect(t3)
        r4, r2, r1 = bc.collect(t4), bc.collect(t2), bc.collect(t1)
        same = lambda got, want: all(g.numpy().tobytes() == w_.tobytes() for g, w_ in zip(got, want))
        assert same(r1, sync["a"]) and same(r2, sync["b"]) and same(r4, sync["a"]), "the neighbours' results changed"
        assert same(r3[0], wh) and same(r3[1], wm), "the asynchronous moves"
        g1, s1, largest, _ = _stats(bc)
        assert (g1 - g0, s1 - s0) == (2, 3) and largest <= 2, "the moves slab must not be a group member"
    finally:
        bc.set_async_depth(2)
        bc.set_coalesce(-1)


def test_decode_split_parts(rv):
    s = SPLIT_SHAPE
    nB, W, Ls = s["B"], s["W"], s["L"]
    bc, _ = _handle(rv, "joint", "luong", 1, SPLIT_SEEDS[0], Tr_max=s["TR"], Te_max=s["TE"], L=Ls, max_batch=nB, end_bias=END_BIAS)
    raw, ev, _ = rv.synthetic.make_slab(nB, s["TR"], s["TE"], seed=SPLIT_SEEDS[1])
    x = _x("joint", raw, ev)
    _set(bc, dict(persistent_decode=0, use_graph=1, decode_split=1))
    h1, m1 = bc.beam_search_moves(x, W, Ls)
    h1, m1 = _np_beams(h1), _np_moves(m1)
    assert (m1.peak[np.arange(h1.tokens.shape[1])[None, :, None] < h1.lengths[:, None, :]] >= 0).all()
    for graph in (1, 0):
        _set(bc, dict(use_graph=graph, decode_split=2))
        h2, m2 = bc.beam_search_moves(x, W, Ls)
        for one, two in ((h1, _np_beams(h2)), (m1, _np_moves(m2))):
            for k in one._fields:
                assert getattr(two, k).tobytes() == getattr(one, k).tobytes() and getattr(two, k).shape == getattr(one, k).shape, \
                    (f"decode_split 2 use_graph {graph}", k)
    bc.close()
