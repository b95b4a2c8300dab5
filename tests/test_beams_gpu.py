"""The whole beam (rv_beam_search_all*, Basecaller.beam_search_hypotheses): all W back-traced hypotheses, the per-slot scores, each
hypothesis's own path scores, and the final state's log_probs and lengths.

k_dec_finalize_beams (csrc/beams.hip) is a pure function of the records the decode leaves, so the expectation is computed from those
records, exactly: after a call the GPU's step_ids / parent_ids / step_scores / chunk_steps are read back through get_tensor and, in
numpy (_expect), every chunk is extended past its own last step with (end_token, identity parent, unchanged score), finished / lengths
are recomputed by TFA's recurrence, the unmodified oracle.gather_tree back-traces every beam, and the slots it passes through give the
path scores.  Integer outputs must be equal and float outputs bit-equal, with no tolerance.  One test (test_against_fp64) then holds
the same outputs to the fp64 oracle, so that the records themselves are the right ones.

Shapes: the B = 6 chunks of test_kernel_forms_gpu._slab (suffix padding, padding after the first step, interior padding, one live
step, two unpadded chunks) in joint mode with T_r = 40, T_e = 8 -- T_m = 48: the second resident row group of the persistent decode
is half padding -- L = 14 and beams 1, 3, 5, 8.

Seeds.  SEEDS[(attention, decoder cells)] = (weight seed, slab seed) of test_kernel_forms_gpu._handle / _slab.  They were searched on
the CPU: for weight seed 1 the slab seeds 1, 2, .. in turn (gain 1.5, end-token bias END_BIAS), taking the first pair at which, for
every beam width the handle is asked for, the oracle's numpy fp32 twin (oracle.beam_search with dtype=np.float32, as
test_parity_gpu._twin_beam runs it) returns the fp64 pass's step ids and parents on all six chunks -- the twin leaves none -- and the
fp64 records are not vacuous in the sense of _assert_not_vacuous: chunks finish at different steps and one before S, some parent is
not the identity, some hypothesis w > 0 differs from hypothesis 0, and the path score of hypothesis 0 differs from the slot-0 score
somewhere (on chunks 0 .. 4, so that the same holds for the slab whose chunk 5 is replaced by padding; such a pair exists for every
handle, so nothing of the list is given up).  Luong and Bahdanau with one cell take (1, 1), the first pair tried; with two cells the
slabs 1 .. 4 have every chunk run all L - 1 steps at some beam width and (1, 5) is the first that does not.  The end-token bias decides
how long the hypotheses are: the weights' logits are nearly flat, at test_kernel_forms_gpu's 0.05 every best hypothesis ends at its
first step and the slab after four, from -0.1 down no chunk ever finishes; at -0.02 the best hypotheses of the fp64 pass are 1 to 13
tokens long and the chunks finish after 2 to 13 steps, so the back-traces are as deep as the shape allows.  SPLIT_SEEDS is the same
search for the B = 70 slab of test_decode_split_parts (synthetic.make_slab): (1, 1), the first pair tried.  test_contract looks at the
columns beyond S, so its slab must stop early: CONTRACT_SEEDS at bias 0.05 (pair (1, 1) runs all 13 steps at beam 5, (1, 2) stops
after 4).  The tests assert non-vacuity on the GPU's own records of
every slab they use before they rely on it."""
import ctypes

import numpy as np
import pytest

from test_config_space_gpu import _filled, _no_sentinel
from test_kernel_forms_gpu import B, PERSIST, _decode_forms, _handle, _set, _slab, _x
from test_parity_gpu import _near_tie_gap

pytestmark = pytest.mark.gpu

TR, TE, L = 40, 8, 14
TM, STEPS = TR + TE, L - 1
TOL = 1e-4
END_BIAS = -0.02
SEEDS = {("luong", 1): (1, 1), ("bahdanau", 1): (1, 1), ("luong", 2): (1, 5)}
CONTRACT_SEEDS, CONTRACT_BIAS = (1, 2), 0.05
SPLIT_SEEDS = (1, 1)
SPLIT_SHAPE = dict(B=70, TR=24, TE=6, L=10, W=5)

PERSIST_OPTS = dict(persistent_decode=1, use_graph=1, decode_split=1)
# form -> (attention, decoder cells, options, the ATT of k_dec_persist it must run or None for the per-step kernels, beam widths)
FORMS = {
    "persistent": ("luong", 1, PERSIST_OPTS, 3, (1, 3, 5, 8)),
    "bahdanau": ("bahdanau", 1, PERSIST_OPTS, 4, (1, 3, 5, 8)),
    "two_cells": ("luong", 2, PERSIST_OPTS, 3, (1, 3, 5)),
    "per_step": ("luong", 1, dict(persistent_decode=0, use_graph=0, decode_split=1), None, (1, 3, 5, 8)),
    "per_step_graph": ("luong", 1, dict(persistent_decode=0, use_graph=1, decode_split=1), None, (1, 3, 5, 8)),
}
CASES = [(f, W) for f, spec in FORMS.items() for W in spec[4]]


# ---------------------------------------------------------------------------------------------- the expectation, from the records
def _expect(oracle, ids, par, sc, cs, end):
    """ids / par [S,B,W] int, sc [S,B,W] f32: the decode's records; cs [B]: the steps each chunk ran (the records of a chunk end
    there).  -> dict(tokens [B,S,W], scores, path_scores, log_probs [B,W], lengths [B,W], slots [B,S,W])."""
    ids, par, sc = ids.astype(np.int32).copy(), par.astype(np.int64).copy(), sc.astype(np.float32).copy()
    S, nB, W = ids.shape
    for b in range(nB):
        c = int(cs[b])
        ids[c:, b] = end
        par[c:, b] = np.arange(W)
        sc[c:, b] = sc[c - 1, b]
    fin, ln = np.zeros((nB, W), bool), np.zeros((nB, W), np.int64)
    fin_at = np.full(nB, S)                  # the step count at which a chunk's beams were all finished
    for s in range(S):                       # TFA: len' = len[parent] + !fin[parent], fin' = fin[parent] | id == end
        pf, pl = np.take_along_axis(fin, par[s], 1), np.take_along_axis(ln, par[s], 1)
        ln, fin = pl + (~pf).astype(np.int64), pf | (ids[s] == end)
        fin_at = np.where(fin.all(axis=1), np.minimum(fin_at, s + 1), fin_at)
    pred = oracle.gather_tree(ids, par, ln.max(axis=1).astype(np.int32), end)
    path = np.zeros((nB, S, W), np.float32)
    slots = np.zeros((nB, S, W), np.int64)
    for b in range(nB):
        Lb = min(S, int(ln[b].max()))
        for w in range(W):
            p = w
            for t in range(Lb - 1, -1, -1):
                slots[b, t, w] = p
                path[b, t, w] = sc[t, b, p]
                p = par[t, b, p]
            slots[b, Lb:, w] = slots[b, Lb - 1, w]
            path[b, Lb:, w] = path[b, Lb - 1, w]
    return dict(tokens=np.transpose(pred, (1, 0, 2)).astype(np.int32), scores=np.ascontiguousarray(np.transpose(sc, (1, 0, 2))),
                path_scores=path, log_probs=sc[S - 1].copy(), lengths=ln.astype(np.int32), slots=slots,
                ids=ids, par=par, cs=np.asarray(cs).astype(int), fin_at=fin_at)


def _assert_not_vacuous(e, W, tag, rows=slice(None), finish_apart=True):
    """The records behind an expectation exercise the kernel: see the module docstring.  finish_apart=False: a slab meant to run every
    chunk to the last step (test_longest_output_gpu's "long" inputs), which states its own condition on the finishing steps."""
    cs, S = e["fin_at"][rows], e["tokens"].shape[1]
    assert not finish_apart or (len(set(cs.tolist())) > 1 and cs.min() < S), (tag, "chunks finish together", cs.tolist(), S)
    if W == 1:
        return
    ident = np.arange(W)[None, None]
    live = np.arange(S)[:, None] < e["fin_at"][None]                  # [S,B]: steps before a chunk's beams were all finished
    assert ((e["par"] != ident).any(axis=2) & live)[:, rows].any(), (tag, "every parent is the identity")
    tok = e["tokens"][rows]
    assert (tok[:, :, 1:] != tok[:, :, :1]).any(), (tag, "every hypothesis equals hypothesis 0")
    assert (e["path_scores"][rows][:, :, 0].view(np.uint32) != e["scores"][rows][:, :, 0].view(np.uint32)).any(), \
        (tag, "the best path sat in slot 0 at every step")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_equal(got, e, tag):
    """BeamHypotheses (cut to S) against an expectation: integers equal, floats bit-equal."""
    for k in ("tokens", "scores", "path_scores", "log_probs", "lengths"):
        g = getattr(got, k)
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        assert g.shape == e[k].shape and g.dtype == e[k].dtype, (tag, k, g.shape, g.dtype, e[k].shape, e[k].dtype)
        assert np.array_equal(_bits(g), _bits(e[k])), (tag, k, np.argwhere(_bits(g) != _bits(e[k]))[:5].tolist())


def _records(bc, S, nB, W, persist):
    t = lambda name, *shape: bc.get_tensor(name).reshape(shape)
    cs = t("chunk_steps", nB).astype(int) if persist else np.full(nB, S)
    return t("step_ids", S, nB, W).astype(int), t("parent_ids", S, nB, W).astype(int), t("step_scores", S, nB, W), cs


def _np_beams(h):
    return type(h)(*[a.cpu().numpy().copy() for a in h])


# ---------------------------------------------------------------------------------------------- handles, slabs, results: made once
_HANDLES, _RESULTS = {}, {}


@pytest.fixture(scope="module")
def handles(rv):
    def get(attention, D):
        if (attention, D) not in _HANDLES:
            wseed, sseed = SEEDS[(attention, D)]
            bc, w = _handle(rv, "joint", attention, D, wseed, Tr_max=TR, Te_max=TE, L=L, end_bias=END_BIAS)
            raw, ev = _slab("joint", TR, TE, seed=sseed)
            praw, pev = raw.copy(), ev.copy()
            praw[5], pev[5] = 0.0, 0.0                # the same slab with its last chunk padding from end to end
            for a in (raw, ev, praw, pev):
                a.setflags(write=False)
            _HANDLES[(attention, D)] = (bc, w, (raw, ev), (praw, pev))
        return _HANDLES[(attention, D)]
    yield get
    for bc, *_ in _HANDLES.values():
        bc.close()
    _HANDLES.clear()
    _RESULTS.clear()


def _result(handles, oracle, form, W):
    """One all-beams call of a form on its slab, with the expectation from its own records (computed once, never modified)."""
    if (form, W) not in _RESULTS:
        attention, D, opts, att, _ = FORMS[form]
        bc, _, (raw, ev), _ = handles(attention, D)
        _set(bc, opts)
        got = _np_beams(bc.beam_search_hypotheses(_x("joint", raw, ev), W, L))
        S = got.tokens.shape[1]
        forms = _decode_forms(bc)
        if att is None:
            assert not any(r[0] == PERSIST for r in forms), (form, W, sorted(forms))
        else:
            assert {r for r in forms if r[0] == PERSIST} == {(PERSIST, W, 2, D, att)}, (form, W, sorted(forms))
        e = _expect(oracle, *_records(bc, S, B, W, att is not None), bc.cfg.end_token)
        _RESULTS[(form, W)] = (got, e, S)
    return _RESULTS[(form, W)]


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("form,W", CASES)
def test_all_beams_equal_gather_tree_of_the_records(handles, oracle, form, W):
    got, e, S = _result(handles, oracle, form, W)
    tag = f"{form} W={W}"
    print(f"{tag}: S = {S}, chunk steps {e['cs'].tolist()}, lengths of hypothesis 0 {e['lengths'][:, 0].tolist()}")
    _assert_not_vacuous(e, W, tag)
    _assert_equal(got, e, tag)


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("form,W", CASES)
def test_slot_zero_is_the_existing_call(handles, oracle, form, W):
    attention, D, opts, att, _ = FORMS[form]
    bc, _, slab, padded = handles(attention, D)
    _set(bc, opts)
    for kind, (raw, ev) in (("slab", slab), ("with a padding chunk", padded)):
        x = _x("joint", raw, ev)
        tok, sc = bc.beam_search_prediction(x, W, L)
        tok, sc = tok.numpy().copy(), sc.numpy().copy()
        got = _np_beams(bc.beam_search_hypotheses(x, W, L))
        tag = f"{form} W={W} {kind}"
        assert got.tokens.shape == (B, tok.shape[1], W), (tag, "S", got.tokens.shape, tok.shape)
        assert got.tokens[:, :, 0].tobytes() == tok.tobytes(), (tag, "tokens")
        assert np.ascontiguousarray(got.scores[:, :, 0]).tobytes() == sc.tobytes(), (tag, "scores")
        if kind != "slab":
            assert np.isnan(sc[5]).all() and tok.shape[1] == STEPS, (tag, "the padding chunk is not one")
            e = _expect(oracle, *_records(bc, STEPS, B, W, att is not None), bc.cfg.end_token)
            _assert_not_vacuous(e, W, tag, rows=slice(0, 5))
            _assert_equal(got, e, tag)


# ---------------------------------------------------------------------------------------------- 3
def _replay(oracle, lg, W, end):
    """The fp64 beam steps over step logits lg [S,B,W,V]: scores [S,B,W], slot-following needs ids / parents of the same pass."""
    nB = lg.shape[1]
    lp = np.full((nB, W), -np.inf); lp[:, 0] = 0.0
    fin, ln = np.zeros((nB, W), bool), np.zeros((nB, W), np.int64)
    ids, par, sc = [], [], []
    for s in range(lg.shape[0]):
        top, word, parent, lp, fin, ln = oracle.beam_search_step(lg[s], lp, fin, ln, end)
        ids.append(word); par.append(parent); sc.append(top)
    return np.stack(ids), np.stack(par), np.stack(sc), ln


@pytest.mark.parametrize("form", ["persistent", "per_step_graph"])
def test_against_fp64(handles, oracle, form):
    W = 5
    attention, D, opts, att, _ = FORMS[form]
    bc, w, (raw, ev), _ = handles(attention, D)
    got, e, S = _result(handles, oracle, form, W)
    end = bc.cfg.end_token
    taps = {}
    oracle.beam_search(w, bc.cfg.oracle_cfg(), raw, ev, W, L, dtype=np.float64, taps=taps)
    oids, opar, osc, oln = _replay(oracle, taps["step_logits"], W, end)
    So = oids.shape[0]
    assert (oids == taps["step_ids"]).all() and (opar == taps["parent_ids"]).all() and (oln == taps["lengths"]).all()
    otok = np.transpose(oracle.gather_tree(taps["step_ids"], taps["parent_ids"], taps["lengths"].max(1), end), (1, 0, 2))
    # the fp64 path scores: the replayed scores along the fp64 back-trace
    opath = np.zeros((B, So, W))
    for b in range(B):
        Lb = min(So, int(oln[b].max()))
        for k in range(W):
            p = k
            for t in range(Lb - 1, -1, -1):
                opath[b, t, k] = osc[t, b, p]
                p = opar[t, b, p]
            opath[b, Lb:, k] = opath[b, Lb - 1, k]
    left = []
    for b in range(B):
        m = min(int(e["cs"][b]), So)
        if (e["ids"][:m, b] != oids[:m, b]).any() or (e["par"][:m, b] != opar[:m, b]).any():
            gap = _near_tie_gap(oracle, taps["step_logits"][:, b], W, end)
            assert gap < TOL, (form, b, "left the fp64 decode with no near-tie", gap)
            left.append(b)
    assert len(left) <= 1, (form, "chunks that left the fp64 decode", left)
    if not left:
        assert S == So, (form, S, So)
    n = min(S, So)
    worst = 0.0
    for b in (b for b in range(B) if b not in left):
        assert (got.tokens[b, :n] == otok[b, :n]).all(), (form, b, "tokens")
        assert (got.lengths[b] == taps["lengths"][b]).all(), (form, b, "lengths", got.lengths[b], taps["lengths"][b])
        err = max(float(np.abs(got.path_scores[b, :n] - opath[b, :n]).max()), float(np.abs(got.log_probs[b] - osc[So - 1, b]).max()))
        worst = max(worst, err)
        assert err < TOL, (form, b, "path_scores / log_probs", err)
    print(f"{form}: S = {S} (fp64 {So}), left {left}, max |path_scores, log_probs - fp64| = {worst:.2e}")


# ---------------------------------------------------------------------------------------------- 5
def test_decode_split_parts(rv, oracle):
    s = SPLIT_SHAPE
    nB, W, Ls = s["B"], s["W"], s["L"]
    bc, _ = _handle(rv, "joint", "luong", 1, SPLIT_SEEDS[0], Tr_max=s["TR"], Te_max=s["TE"], L=Ls, max_batch=nB, end_bias=END_BIAS)
    raw, ev, _ = rv.synthetic.make_slab(nB, s["TR"], s["TE"], seed=SPLIT_SEEDS[1])
    x = _x("joint", raw, ev)
    _set(bc, dict(persistent_decode=0, use_graph=1, decode_split=1))
    one = _np_beams(bc.beam_search_hypotheses(x, W, Ls))
    S = one.tokens.shape[1]
    e = _expect(oracle, *_records(bc, S, nB, W, False), bc.cfg.end_token)
    _assert_not_vacuous(e, W, "decode_split 1")
    _assert_equal(one, e, "decode_split 1")
    for graph in (1, 0):
        _set(bc, dict(use_graph=graph, decode_split=2))
        two = _np_beams(bc.beam_search_hypotheses(x, W, Ls))
        for k in one._fields:
            assert getattr(two, k).tobytes() == getattr(one, k).tobytes() and getattr(two, k).shape == getattr(one, k).shape, \
                (f"decode_split 2 use_graph {graph}", k)
    bc.close()


# ---------------------------------------------------------------------------------------------- 6
def _stats(bc):
    return [int(v) for v in bc.get_tensor("coalesce_stats")]


def _same_pair(got, want):
    return all(np.asarray(g.cpu() if hasattr(g, "cpu") else g).tobytes() == w.tobytes() for g, w in zip(got, want))


def test_async_and_device_outputs(rv, handles, oracle):
    import torch
    bc, _, slab, padded = handles("luong", 1)
    _set(bc, PERSIST_OPTS)
    xs = {"a": _x("joint", *slab), "b": _x("joint", *padded)}
    dev = {k: tuple(torch.from_numpy(a.copy()).cuda() for a in v) for k, v in xs.items()}
    sync = {(k, W): tuple(t.numpy().copy() for t in bc.beam_search_prediction(xs[k], W, L)) for k in xs for W in (5, 3)}
    sync_all = {(k, W): _np_beams(bc.beam_search_hypotheses(xs[k], W, L)) for k in xs for W in (5, 3)}
    bc.set_async_depth(4)
    bc.set_coalesce(2)
    try:
        g0, s0, _, in_force = _stats(bc)
        assert in_force == 2
        mine = bc._beams_dev(B, STEPS, 3)
        for t in mine:
            t.view(torch.int32).fill_(0x7F7F7F7F)
        t1 = bc.submit_beam_search(xs["a"], 5, L)                              # ordinary: a group of two ...
        t2 = bc.submit_beam_search(xs["b"], 5, L)                              # ... which launches full
        t3 = bc.submit_beam_search(xs["b"], 5, L, all_beams=True)              # the whole beam, host results
        t4 = bc.submit_beam_search(dev["a"], 3, L, all_beams=True, out=mine)   # the whole beam into the caller's device tensors
        with pytest.raises(rv._capi.RavventHipError, match="RV_ESTATE"):       # four tickets out, four contexts: refused, touching nothing
            bc.beam_search_hypotheses(xs["a"], 5, L)
        with pytest.raises(rv._capi.RavventHipError, match="RV_ESTATE"):
            bc.submit_beam_search(xs["a"], 5, L, all_beams=True)
        r4 = bc.collect(t4)
        t5 = bc.submit_beam_search(xs["a"], 3, L)                              # ordinary: opens a group that never fills
        r2 = bc.collect(t2)
        between = _np_beams(bc.beam_search_hypotheses(xs["a"], 3, L))          # synchronous, between tickets: an idle context
        r3 = bc.collect(t3)
        r5 = bc.collect(t5)
        r1 = bc.collect(t1)
        assert _same_pair(r1, sync[("a", 5)]) and _same_pair(r2, sync[("b", 5)]) and _same_pair(r5, sync[("a", 3)])
        for got, want, tag in ((r3, sync_all[("b", 5)], "host"), (r4, sync_all[("a", 3)], "device"), (between, sync_all[("a", 3)], "synchronous")):
            assert type(got).__name__ == "BeamHypotheses"
            for k in want._fields:
                g = getattr(got, k)
                g = g.cpu().numpy() if hasattr(g, "cpu") else g
                assert g.shape == getattr(want, k).shape and g.tobytes() == getattr(want, k).tobytes(), (tag, k)
        S4 = sync_all[("a", 3)].tokens.shape[1]
        assert r4.tokens.data_ptr() == mine.tokens.data_ptr() and r4.tokens.shape[1] == S4
        _no_sentinel(*[t.cpu().numpy() for t in mine])
        g1, s1, largest, _ = _stats(bc)
        assert (g1 - g0, s1 - s0) == (2, 3) and largest <= 2, "the all-beams slabs must not be group members"
    finally:
        bc.set_async_depth(2)
        bc.set_coalesce(-1)


# ---------------------------------------------------------------------------------------------- 7
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _host_bufs(nB, W, steps=STEPS):
    return [_filled((nB, steps, W), np.int32), _filled((nB, steps, W), np.float32), _filled((nB, steps, W), np.float32),
            _filled((nB, W), np.float32), _filled((nB, W), np.int32)]


def test_contract(rv, handles, oracle):
    import torch
    bc, _ = _handle(rv, "joint", "luong", 1, CONTRACT_SEEDS[0], Tr_max=TR, Te_max=TE, L=L, end_bias=CONTRACT_BIAS)
    raw, ev = _slab("joint", TR, TE, seed=CONTRACT_SEEDS[1])
    lib, h, S = bc._lib, bc._h, ctypes.c_int32(-1)
    W = 5
    pad_token, end = bc.cfg.pad_token, bc.cfg.end_token
    struct = lambda bufs: rv._capi.CRvBeams(*[_p(a) for a in bufs])
    call = lambda bufs, nB=B, Lc=L, Wc=W: lib.rv_beam_search_all(h, _p(raw), _p(ev), nB, TR, TE, Wc, Lc, ctypes.byref(struct(bufs)), ctypes.byref(S))
    d_raw, d_ev = torch.from_numpy(raw.copy()).cuda(), torch.from_numpy(ev.copy()).cuda()
    dp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    for opts in (PERSIST_OPTS, dict(persistent_decode=0, use_graph=1, decode_split=1)):
        _set(bc, opts)
        # host buffers
        bufs = _host_bufs(B, W)
        bc._check(call(bufs), "rv_beam_search_all")
        Sv = S.value
        assert 0 < Sv < STEPS, (opts, "badly chosen: the slab runs all its steps", Sv)
        tok, sc, path, lp, ln = bufs
        e = _expect(oracle, *_records(bc, Sv, B, W, bool(opts["persistent_decode"])), end)
        for k, a in zip(("tokens", "scores", "path_scores"), (tok, sc, path)):
            assert np.array_equal(_bits(a[:, :Sv]), _bits(e[k])), (opts, k)
        assert np.array_equal(_bits(lp), _bits(e["log_probs"])) and np.array_equal(ln, e["lengths"])
        assert (tok[:, Sv:] == pad_token).all(), (opts, "tokens beyond S")
        assert (sc[:, Sv:].view(np.uint32) == 0).all() and (path[:, Sv:].view(np.uint32) == 0).all(), (opts, "scores beyond S")
        _no_sentinel(*bufs)
        # device buffers: the same bytes
        dbufs = [torch.full(a.shape, 0x7F7F7F7F, dtype=torch.int32, device="cuda") for a in bufs]
        st = rv._capi.CRvBeams(*[dp(t) for t in dbufs])
        bc._check(lib.rv_beam_search_all_dev(h, dp(d_raw), dp(d_ev), B, TR, TE, W, L, ctypes.byref(st), ctypes.byref(S)), "rv_beam_search_all_dev")
        assert S.value == Sv
        for a, t in zip(bufs, dbufs):
            assert t.cpu().numpy().tobytes() == a.tobytes(), (opts, "device outputs differ from host outputs")
        # NULL optional outputs: accepted, the others unchanged
        for drop in ((2,), (3,), (4,), (2, 3, 4)):
            part = _host_bufs(B, W)
            for i in drop:
                part[i] = None
            bc._check(call(part), "rv_beam_search_all")
            assert S.value == Sv
            for a, b_ in zip(part, bufs):
                assert a is None or a.tobytes() == b_.tobytes(), (opts, drop)
            dpart = [None if i in drop else torch.full(a.shape, 0x7F7F7F7F, dtype=torch.int32, device="cuda") for i, a in enumerate(bufs)]
            st = rv._capi.CRvBeams(*[dp(t) for t in dpart])
            bc._check(lib.rv_beam_search_all_dev(h, dp(d_raw), dp(d_ev), B, TR, TE, W, L, ctypes.byref(st), ctypes.byref(S)), "rv_beam_search_all_dev")
            for t, b_ in zip(dpart, bufs):
                assert t is None or t.cpu().numpy().tobytes() == b_.tobytes(), (opts, drop, "device")
        # NULL required outputs
        for i in (0, 1):
            part = _host_bufs(B, W)
            part[i] = None
            assert call(part) == -1, "RV_EINVAL expected"
            assert b"null output pointer" in lib.rv_last_error(h)
            dpart = list(dbufs)
            dpart[i] = None
            st = rv._capi.CRvBeams(*[dp(t) for t in dpart])
            assert lib.rv_beam_search_all_dev(h, dp(d_raw), dp(d_ev), B, TR, TE, W, L, ctypes.byref(st), ctypes.byref(S)) == -1
        assert lib.rv_beam_search_all(h, _p(raw), _p(ev), B, TR, TE, W, L, None, ctypes.byref(S)) == -1
    _set(bc, PERSIST_OPTS)
    # a beam wider than the handle's: the message of rv_beam_search
    narrow = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=B, max_raw_len=TR, max_event_len=TE,
                           max_output_len=L, max_beam=3)
    narrow.init_random_weights(seed=1)
    with pytest.raises(rv._capi.RavventHipError, match=r"RV_EINVAL: beam width 5 outside \[1,3\]"):
        narrow.beam_search_hypotheses(_x("joint", raw, ev), 5, L)
    with pytest.raises(rv._capi.RavventHipError, match=r"RV_EINVAL: beam width 5 outside \[1,3\]"):
        narrow.beam_search_prediction(_x("joint", raw, ev), 5, L)
    narrow.close()
    # trivial calls: nothing runs, S = 0, the initial state
    init_lp = np.tile(np.array([0.0] + [-np.inf] * (W - 1), np.float32), (B, 1))
    bufs = _host_bufs(B, W, steps=0)
    bc._check(call(bufs, Lc=1), "rv_beam_search_all L=1")
    assert S.value == 0 and np.array_equal(_bits(bufs[3]), _bits(init_lp)) and (bufs[4] == 0).all()
    dlp = torch.full((B, W), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    dln = torch.full((B, W), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    st = rv._capi.CRvBeams(None, None, None, dp(dlp), dp(dln))
    bc._check(lib.rv_beam_search_all_dev(h, dp(d_raw), dp(d_ev), B, TR, TE, W, 1, ctypes.byref(st), ctypes.byref(S)), "rv_beam_search_all_dev L=1")
    assert S.value == 0 and np.array_equal(dlp.cpu().numpy().view(np.uint32), _bits(init_lp)) and (dln.cpu().numpy() == 0).all()
    bufs = _host_bufs(0, W)
    S.value = -1
    bc._check(call(bufs, nB=0), "rv_beam_search_all B=0")
    assert S.value == 0
    hyp = bc.beam_search_hypotheses(_x("joint", raw[:0], ev[:0]), W, L)
    assert hyp.tokens.shape == (0, 0, W) and hyp.log_probs.shape == (0, W)
    hyp = bc.beam_search_hypotheses(_x("joint", raw, ev), W, 1)
    assert hyp.tokens.shape == (B, 0, W) and np.array_equal(_bits(hyp.log_probs.numpy()), _bits(init_lp)) and (hyp.lengths.numpy() == 0).all()
    bc.close()


# ---------------------------------------------------------------------------------------------- the Python helpers
def test_strings_and_probabilities_of_every_hypothesis(rv, handles, oracle):
    got, e, S = _result(handles, oracle, "persistent", 5)
    bc = handles("luong", 1)[0]
    strings = bc.tokens_to_nuc_sequences(got.tokens)
    assert len(strings) == B and all(len(row) == 5 for row in strings)
    for k in range(5):
        assert [row[k] for row in strings] == oracle.tokens_to_nuc_sequences(got.tokens[:, :, k])
    assert [row[0] for row in strings] == bc.tokens_to_nuc_sequences(got.tokens[:, :, 0])
    probs = rv.utils.calc_prob_path_scores(got.path_scores)
    want = np.stack([oracle.calc_prob_logits_beam_search_scores(got.path_scores[:, :, k]) for k in range(5)], axis=2)
    assert probs.shape == (B, S, 5) and np.array_equal(probs, want)
    live = np.arange(S)[None, :, None] < e["lengths"][:, None, :]
    assert (probs[live] <= 1.0 + 1e-6).all() and (probs[live] > 0).all(), "a hypothesis's own steps carry probabilities"
    # the torch form: the same differences, exp by another library -- each faithful to an ulp, and no probability exceeds 1
    import torch
    assert np.abs(rv.utils.calc_prob_path_scores(torch.from_numpy(got.path_scores)).numpy() - probs).max() <= 2 * np.finfo(np.float32).eps
