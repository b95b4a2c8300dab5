"""rnn_type='bigru' on the GPU against the numpy reference of tests/gru_reference.py (fp64, and its fp32 twin for the twin-relative bound).

The cases (tests/gru_cases.py; tests/test_gru.py proves on the reference alone that each is a fair probe) are sized to where the new
kernels can go wrong:
  rows-*    k_gru_rec_mx's chunk rows: a lone chunk, a full workgroup of sixteen, one live row beside fifteen clamped ones; raw (F = 1)
            and event (F = 5) layer-0 forms;
  tail-*    the step loop's triples and its one- or two-step tail, T = 1..5, both directions starting on their edge; F = 0 behind them;
  chain-*   layer l + 1 starting from layer l's final states, and the three-block input GEMM at M = 119 (a partial row tile), 300, 60;
  cell-*    k_dec_cell_gru's 64-row workgroup at N = B W = 1, 64, 65, one to three stacked cells, both attentions;
  search-*  greedy and beam 1, 2, 5, 8 on one slab of seventeen chunks;
  allpad-*  one chunk that is padding from end to end: NaN where the reference has NaN, its neighbours untouched;
  lds-*     the layer-0 event form's dynamic LDS on either side of 64 KB (T_e = 115, 116: where the opt-in of configure_gru_kernels starts to
            matter) and at the decode's 352 steps;
  long-*    the F = 1 form and the F = 0 input ring over 352 steps, the chunker's 200 + 30 (k = 2 of the three-block GEMM), 100 + 252 with
            T_m = 352 through the per-step attend, and the two-pass Bahdanau attend at T_m = 352 under a GRU cell;
  gemm-k5   raw M = 13,000: the three-block GEMM with k = 5 row-group multiples, the geometry of the shipped 1024 x 200 shape.
Every case holds enc_output, mask, keys, step logits and step alignments to TOL of fp64 and to TWIN_K x the fp32 twin + TWIN_C; a
chunk may leave the fp64 decode only through a near-tie narrower than twice the logits bound.  Then the outer interfaces, one case each,
the refusals (options; windows that do not fit the 160 KB of LDS, both sides of each edge), and adversarial weights: the split-f16 image
of U and the 2^14 image of h under large and tiny rows, gained columns and saturated activations; the decoder cell under a gain of 50."""
import numpy as np
import pytest

import gru_cases as C
import gru_reference as G
from test_bench_config_gpu import TWIN_C, TWIN_K
from test_parity_gpu import TOL, _assert_twin, _beam_errors, _greedy_errors, _memory_errors, _near_tie_gap

pytestmark = pytest.mark.gpu


def _open(rv, c, **kw):
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, c.mode, 0.0, encoder_depth=c.enc_depth, decoder_depth=c.dec_depth,
                       rnn_type="bigru", attention_type=c.attention, honor_attention_type=True, max_batch=kw.get("max_batch", c.B),
                       max_raw_len=max(c.Tr, 1), max_event_len=max(c.Te, 1), max_output_len=kw.get("L", c.L), max_beam=kw.get("max_beam", max(c.W, 1)))
    flat = kw.get("flat") or C.weights(rv, c.enc_depth, c.dec_depth, c.mode, c.attention)[0]
    bc.set_weights_flat(flat)
    return bc


def _x(mode, raw, ev):
    return {"joint": (raw, ev), "raw": raw, "event": ev}[mode]


def _tie_bound(twin):
    """What the logits bound allows: two candidates closer than this can be ordered either way by an evaluation that meets it."""
    return 2 * (TWIN_K * twin["step_logits"] + TWIN_C)


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_case_against_fp64_and_twin(rv, name):
    c, r = C.BY_NAME[name], C.fp64(rv, name)
    twin = C.twin_errors(rv, name)
    keep = C.keep_rows(c)
    o_out, o = C.sliced(r["out"], r["taps"], keep)
    raw, ev, B = r["raw"], r["ev"], c.B
    Tm = r["taps"]["mask"].shape[1]
    bc = _open(rv, c)
    bc.set_option("debug_taps", 1)
    if c.W == 0:
        tok, lg = (a.numpy() for a in bc.greedy_search_prediction(_x(c.mode, raw, ev), c.L))
    else:
        tok, sc = (a.numpy() for a in bc.beam_search_prediction(_x(c.mode, raw, ev), c.W, c.L))
    S = tok.shape[1]
    enc = bc.get_tensor("enc_output").reshape(B, Tm, 256)
    keys = bc.get_tensor("keys").reshape(B, Tm, 128)
    assert (bc.get_tensor("mask").reshape(B, Tm) == r["taps"]["mask"]).all(), name
    err = _memory_errors(enc, keys, r["taps"])                       # every chunk: an all-padding chunk's encoder output is ordinary numbers
    forms = {tuple(int(v) for v in row) for row in bc.get_tensor("kernel_forms").reshape(-1, 5)}
    want = {(9, F, 16, 0, 0) for F in ([1] if c.mode != "event" else []) + ([5] if c.mode != "raw" else []) + ([0] if c.enc_depth > 1 else [])}
    assert {f for f in forms if f[0] == 9} == want and (10, 0, 0, 0, 0) in forms, (name, sorted(forms))
    assert not any(f[0] in (0, 3, 4, 5, 6, 7, 8) for f in forms), (name, "an LSTM kernel ran on a GRU handle", sorted(forms))
    if c.W == 0:
        og, olg = o_out
        al = bc.get_tensor("step_alignments").reshape(S, B, 1, Tm)[:, :, 0]
        e, left = _greedy_errors(tok[keep], lg[keep], al[:, keep], og, olg, o)
        for i in left:                                                # a token differs: only at a near-tie of the fp64 logits
            s = int(np.nonzero(tok[keep][i, :S] != og[i, :S])[0][0])
            top2 = np.sort(olg[i, s])[-2:]
            assert top2[1] - top2[0] < _tie_bound(twin), (name, keep[i], s, "a greedy token differs with no near-tie", float(top2[1] - top2[0]))
        if not left:
            assert S == r["out"][0].shape[1], (name, S)
        same = [i for i in range(len(keep)) if i not in left]
        assert bc.tokens_to_nuc_sequences(tok[keep][same]) == G.tokens_to_nuc_sequences(og[same]), name
        if c.all_pad is not None:
            assert np.isnan(lg[c.all_pad]).all() and np.isnan(al[:, c.all_pad]).all() and (tok[c.all_pad] == 0).all(), name
    else:
        otok, osc = o_out
        W, V = c.W, 7
        lgs = bc.get_tensor("step_logits").reshape(S, B, W, V)
        al = bc.get_tensor("step_alignments").reshape(S, B, W, Tm)
        ids = bc.get_tensor("step_ids").reshape(S, B, W).astype(np.int64)
        par = bc.get_tensor("parent_ids").reshape(S, B, W).astype(np.int64)
        e, left = _beam_errors(lgs[:, keep], al[:, keep], ids[:, keep], par[:, keep], np.full(len(keep), S), sc[keep], o, osc)
        for i in left:
            gap = _near_tie_gap(G, o["step_logits"][:, i], W, r["cfg"]["end_token"])
            assert gap < _tie_bound(twin), (name, keep[i], "left the fp64 beam with no near-tie", gap)
        n = min(S, otok.shape[1])
        for i in (i for i in range(len(keep)) if i not in left):
            assert (tok[keep[i], :n] == otok[i, :n]).all(), (name, keep[i], "tokens")
        if not left:
            assert S == r["out"][0].shape[1], (name, S)
        if c.all_pad is not None:
            assert np.isnan(sc[c.all_pad]).all() and (tok[c.all_pad] == 0).all() and np.isnan(al[:, c.all_pad]).all(), name
            assert np.array_equal(np.isnan(sc), np.isnan(r["out"][1])), name
    assert len(left) <= len(keep) // 4, (name, "chunks that left the fp64 decode", left)
    err.update(e)
    print(f"{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) + f"; chunks that left the fp64 decode: {[keep[i] for i in left]}")
    for k, v in err.items():
        assert v < TOL, (name, k, v)
    _assert_twin(err, twin, name)
    bc.close()


# ---------------------------------------------------------------------------------------------- the outer interfaces
WORLD = C.WORLD


@pytest.fixture(scope="module")
def world(rv):
    """One joint handle of two encoder layers (max_beam 8), the slab of case world-beam5, its synchronous beam search of width 5 and the
    fp64 reference of it, computed once and left as they are."""
    import torch
    bc = _open(rv, WORLD, max_beam=8)
    r = C.fp64(rv, WORLD.name)
    dev = (torch.from_numpy(r["raw"].copy()).cuda(), torch.from_numpy(r["ev"].copy()).cuda())
    tok, sc = (a.numpy().copy() for a in bc.beam_search_prediction((r["raw"], r["ev"]), 5, WORLD.L))
    for a in (tok, sc):
        a.setflags(write=False)
    yield dict(bc=bc, raw=r["raw"], ev=r["ev"], w=r["w"], cfg=r["cfg"], tok=tok, sc=sc, otok=r["out"][0], osc=r["out"][1], taps=r["taps"], dev=dev)
    bc.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def test_sync_call_matches_fp64(world):
    S = world["otok"].shape[1]
    assert world["tok"].shape == (WORLD.B, S) and (world["tok"] == world["otok"]).all()
    assert np.abs(world["sc"] - world["osc"]).max() < TOL


def test_all_beams(world):
    """rv_beam_search_all: hypotheses, path scores and lengths against the reference's records (test_beams_gpu._expect back-traces them)."""
    from test_beams_gpu import _expect
    bc, t = world["bc"], world["taps"]
    hyp = bc.beam_search_hypotheses((world["raw"], world["ev"]), 5, WORLD.L)
    S = t["step_ids"].shape[0]
    e = _expect(G, t["step_ids"], t["parent_ids"], t["step_scores"], np.full(WORLD.B, S), world["cfg"]["end_token"])
    assert hyp.tokens.shape == (WORLD.B, S, 5)
    assert (hyp.tokens.numpy() == e["tokens"]).all() and (hyp.lengths.numpy() == t["lengths"]).all()
    assert np.abs(hyp.path_scores.numpy() - e["path_scores"]).max() < TOL and np.abs(hyp.scores.numpy() - e["scores"]).max() < TOL
    assert np.abs(hyp.log_probs.numpy() - t["log_probs"]).max() < TOL
    assert np.array_equal(hyp.tokens.numpy()[:, :, 0], world["tok"]) and np.array_equal(_bits(hyp.scores.numpy()[:, :, 0]), _bits(world["sc"]))


def test_teacher_forced_logits_and_nll(rv, world):
    from test_teacher_forced import np_nll
    bc = world["bc"]
    rng = np.random.default_rng(9)
    L = WORLD.L
    target = rng.integers(3, 7, (WORLD.B, L)).astype(np.int32)
    target[:, 0] = bc.cfg.start_token
    target[3, 7:] = bc.cfg.pad_token                                  # padding labels: nll 0 there
    target[5, 4] = bc.cfg.end_token
    ids, ref = G.greedy_search(world["w"], world["cfg"], world["raw"], world["ev"], L, forced=target)
    _, tw = G.greedy_search(world["w"], world["cfg"], world["raw"], world["ev"], L, dtype=np.float32, forced=target)
    r = bc._teacher_forced((world["raw"], world["ev"]), target, bc._train_omit)
    lg = r.logits.numpy()
    assert lg.shape == ref.shape == (WORLD.B, L - 1, 7)
    e_gpu, e_tw = float(np.abs(lg - ref).max()), float(np.abs(tw - ref).max())
    bound = min(TOL, TWIN_K * e_tw + TWIN_C)
    print(f"forced logits: max |gpu - fp64| {e_gpu:.2e}, twin {e_tw:.2e}")
    assert e_gpu <= bound
    agree = np.sort(ref, -1)[..., -1] - np.sort(ref, -1)[..., -2] >= 2 * bound
    assert (r.sample_id.numpy()[agree] == ids[agree]).all()
    real = target[:, 1:]
    nll = r.nll.numpy()
    assert np.abs(nll - np_nll(ref, real)).max() <= 2 * bound and (nll[real == bc.cfg.pad_token] == 0).all()
    want = np.zeros(WORLD.B, np.float32)
    for s in range(L - 1):
        want = want + nll[:, s]
    assert np.array_equal(r.nll_sum.numpy(), want)
    assert np.abs(r.nll_sum.numpy() - np_nll(ref, real).sum(1)).max() <= 2 * bound * (L - 1)


def test_asynchronous_calls_equal_the_synchronous_call(world):
    bc = world["bc"]
    bc.set_async_depth(2)
    stats0 = bc.get_tensor("coalesce_stats")[0]
    tickets = [bc.submit_beam_search(world["dev"], 5, WORLD.L), bc.submit_beam_search((world["raw"], world["ev"]), 5, WORLD.L)]
    for t in tickets:
        tok, sc = bc.collect(t)
        assert np.array_equal(tok.cpu().numpy(), world["tok"]) and np.array_equal(_bits(sc.cpu().numpy()), _bits(world["sc"]))
    assert bc.get_tensor("coalesce_stats")[0] == stats0, "a GRU handle's slabs are never coalesced"


def test_window_table_equals_expanded_rows(rv, world):
    bc = world["bc"]
    rng = np.random.default_rng(4)
    n_raw, n_ev = 400, 60
    read = (rng.standard_normal(n_raw).astype(np.float32), rng.standard_normal((n_ev, 5)).astype(np.float32))
    rows = np.array([(0, 50, 0, 7), (n_raw - 50, 50, n_ev - 7, 7), (n_raw - 17, 17, n_ev - 3, 3), (5, 0, 4, 5), (11, 23, 9, 0)] +
                    [(2 + 3 * i, 50 - i % 7, 2 + i, 7 - i % 3) for i in range(12)], np.int32)
    assert rows.shape == (WORLD.B, 4)
    handle = bc.put_read(*read)
    raw, ev = rv.data_loader.expand_windows(read[0], read[1], rows, 50, 7, 0.0)
    tok, sc = (a.numpy().copy() for a in bc.beam_search_prediction((raw, ev), 5, WORLD.L))
    e0 = bc.get_tensor("read_stats")[4]
    wt, ws = bc.beam_search_windows(handle.table(rows), 5, WORLD.L, T_r=50, T_e=7)
    assert np.array_equal(wt.numpy(), tok) and np.array_equal(_bits(ws.numpy()), _bits(sc))
    assert bc.get_tensor("read_stats")[4] == e0 + 1, "a GRU handle's window call runs behind k_expand_windows"
    handle.drop()


def test_basecall_of_a_short_read(rv):
    dl = rv.data_loader
    c = C._c("basecall", 16, "joint", dl.MAX_RAW_LEN, dl.MAX_EVENT_LEN, enc_depth=2, W=5, L=24)
    bc = _open(rv, c)
    flat, _ = C.weights(rv, 2, 1, "joint", "luong")
    flat = {k: v.copy() for k, v in flat.items()}
    flat["b_fc"][3:7] += 1.5                                          # call bases: a string to merge
    flat["b_fc"][bc.cfg.end_token] -= 3.0
    bc.set_weights_flat(flat)
    sig, _ = rv.synthetic.make_read(n_bases=60, seed=3)
    res = bc.basecall(sig, chunk_size=16)
    rw = dl.prepare_windows(sig, stride=6)
    raw, ev = rw.expand()
    n = len(rw)
    parts = [bc.beam_search_call_arrays((raw[a:a + 16], ev[a:a + 16]), 5, 24) for a in range(0, n, 16)]
    seq, probs = rv.merger.Merger().merge_arrays(*[np.concatenate([p[k] for p in parts]) for k in range(3)])
    assert res.chunks_num == n and len(seq) > 10 and res.seq == seq and res.probs.tobytes() == probs.tobytes()
    bc.close()


def test_use_graph_0_equals_1(world):
    bc = world["bc"]
    try:
        bc.set_option("use_graph", 0)
        tok, sc = (a.numpy().copy() for a in bc.beam_search_prediction((world["raw"], world["ev"]), 5, WORLD.L))
    finally:
        bc.set_option("use_graph", 1)
    assert np.array_equal(tok, world["tok"]) and np.array_equal(_bits(sc), _bits(world["sc"]))


def test_moves_against_the_reference_alignments(rv, world):
    """tests/moves_reference.py takes the GRU reference's taps as they are (alignments, ids, parents, lengths).  Bounds from the
    alignments' own bound per element, d = TWIN_K x the fp32 twin's alignment error on this slab + TWIN_C (what the case test holds
    the GPU's alignments to), as tests/test_moves_gpu.py derives them from its measured d: a mass over n steps within
    n d (+ fp32 summation), a position m1 / m0 within n^2 d / (2 m0) (+ rounding), the peak on a weight within 2 d of the largest."""
    import moves_reference as M
    bc, t = world["bc"], world["taps"]
    hyp, mv = bc.beam_search_moves((world["raw"], world["ev"]), 5, WORLD.L)
    assert np.array_equal(hyp.tokens.numpy()[:, :, 0], world["tok"]) and (hyp.lengths.numpy() == t["lengths"]).all()
    a64, par, ln = t["step_alignments"], t["parent_ids"], t["lengths"]
    ref = M.moves_reference(a64, t["step_ids"], par, ln, WORLD.Tr, world["cfg"]["end_token"])
    slot, _ = M.slots(par, ln)
    d = TWIN_K * C.twin_errors(rv, WORLD.name)["step_alignments"] + TWIN_C      # the bound this slab's alignments are held to (test_case_against_fp64_and_twin)
    S, Tm, u = a64.shape[0], WORLD.Tr + WORLD.Te, 2.0 ** -24
    print(f"moves: alignment bound d = {d:.2e}")
    live = np.arange(S)[None, :, None] < ln[:, None, :]
    assert live.sum() > WORLD.B * 5
    for seg, n in (("raw", WORLD.Tr), ("event", WORLD.Te)):
        m64, p64 = ref[seg + "_mass"], ref[seg + "_pos"]
        mg, pg = getattr(mv, seg + "_mass").numpy(), getattr(mv, seg + "_pos").numpy()
        assert (m64[live] > 0).all(), "no segment of this slab is masked out whole"
        assert (np.abs(mg - m64)[live] <= n * d + (Tm + 2) * 2 * u).all(), seg
        assert (np.abs(pg - p64)[live] <= n * n * d / (2 * m64[live]) + 2 * (Tm + 2) * u * np.abs(p64[live])).all(), seg
        assert (mg[~live] == 0).all() and (pg[~live] == -1).all(), seg
    pk, pw = mv.peak.numpy(), mv.peak_weight.numpy()
    for b, tt, k in zip(*np.nonzero(live)):
        row = a64[tt, b, int(par[tt, b, slot[b, tt, k]])]
        assert 0 <= pk[b, tt, k] < Tm and row[pk[b, tt, k]] >= row.max() - 2 * d, (b, tt, k)
        assert abs(pw[b, tt, k] - row.max()) <= d, (b, tt, k)
    assert (pk[~live] == -1).all() and (pw[~live] == 0).all()


# ---------------------------------------------------------------------------------------------- a BiLSTM handle beside
_BESIDE = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import ravvent_basecaller_amd as rv
import gru_cases as C
c = C.WORLD
raw, ev = C.slab(rv, c)
lstm = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=2, max_batch=c.B, max_raw_len=c.Tr,
                     max_event_len=c.Te, max_output_len=c.L)
lstm.init_random_weights(seed=22)
run = lambda: [a.numpy().copy() for a in lstm.beam_search_prediction((raw, ev), 5, c.L)]
before = run()                                   # no GRU handle has existed in this process
gru = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=2, rnn_type="bigru", max_batch=c.B,
                    max_raw_len=c.Tr, max_event_len=c.Te, max_output_len=c.L)
created = run()                                  # created: its kernels configured, its buffers allocated
gru.set_weights_flat(C.weights(rv, 2, 1, "joint", "luong")[0])
gtok, _ = gru.beam_search_prediction((raw, ev), 5, c.L)
used = run()
gru.close()
closed = run()
for tag, got in (("created", created), ("used", used), ("closed", closed)):
    assert got[0].shape == before[0].shape and got[0].tobytes() == before[0].tobytes() and got[1].tobytes() == before[1].tobytes(), tag
assert before[0].shape[1] >= 2 and gtok.shape[0] == c.B
print("beside ok", before[0].shape, gtok.shape)
"""


def test_a_bilstm_handle_returns_its_bytes_across_the_life_of_a_gru_handle():
    """In a process of its own, so that the BiLSTM handle's first call precedes the first GRU handle of the process whatever ran before
    this test: the same bytes before the GRU handle is created, once it exists, after it has decoded and after it is closed."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable, *flags, "-c", _BESIDE, os.path.dirname(here), here], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "beside ok" in p.stdout, (p.returncode, p.stdout[-400:], p.stderr[-1500:])


# ---------------------------------------------------------------------------------------------- refusals
def test_refused_options_and_a_bilstm_handle_beside(rv, world):
    """Each option no GRU kernel stands behind is RV_EUNSUPPORTED with the family's name, and the handle works on.  LSTM-only and
    persistent-decode options are accepted and inert.  A BiLSTM handle of the same process keeps its bytes and its form list through
    all of it (its bytes across the creation of a GRU handle: the test above)."""
    lstm = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=2, max_batch=WORLD.B, max_raw_len=50,
                         max_event_len=7, max_output_len=WORLD.L)
    lstm.init_random_weights(seed=22)
    before = [a.numpy().copy() for a in lstm.beam_search_prediction((world["raw"], world["ev"]), 5, WORLD.L)]
    bc = world["bc"]
    for key, value in (("weight_parts", 1), ("wide_recurrence", 0), ("wide_recurrence", -1), ("wide_recurrence", 2), ("lane_projection", 0),
                       ("slab_graph", 1)):
        with pytest.raises(rv._capi.RavventHipError) as e:
            bc.set_option(key, value)
        assert "RV_EUNSUPPORTED" in str(e.value) and "bigru" in str(e.value) and key in str(e.value), (key, str(e.value))
        tok, sc = (a.numpy() for a in bc.beam_search_prediction((world["raw"], world["ev"]), 5, WORLD.L))
        assert np.array_equal(tok, world["tok"]) and np.array_equal(_bits(sc), _bits(world["sc"])), key
    with pytest.raises(rv._capi.RavventHipError) as e:
        bc.set_weight_parts(1)
    assert "RV_EUNSUPPORTED" in str(e.value) and bc.weight_parts == 2
    try:
        for key, value in (("persistent_decode", 1), ("matrix_attention", 0), ("matrix_cell", 0), ("fused_memory", 0), ("tail_wave", 0),
                           ("fused_projection", 0), ("split_projection", 0), ("wide_recurrence", 1), ("lane_projection", 1),
                           ("weight_parts", 2), ("slab_graph", 0)):
            bc.set_option(key, value)
            tok, sc = (a.numpy() for a in bc.beam_search_prediction((world["raw"], world["ev"]), 5, WORLD.L))
            assert np.array_equal(tok, world["tok"]) and np.array_equal(_bits(sc), _bits(world["sc"])), key
    finally:
        for key, value in (("matrix_attention", 1), ("matrix_cell", 1), ("fused_memory", 1), ("tail_wave", 1), ("fused_projection", 1),
                           ("split_projection", 2)):
            bc.set_option(key, value)
    listed = {tuple(int(v) for v in row) for row in bc.get_tensor("kernel_form_list").reshape(-1, 5)}
    assert {(9, 0, 16, 0, 0), (9, 1, 16, 0, 0), (9, 5, 16, 0, 0), (10, 0, 0, 0, 0)} <= listed and not any(f[0] in (0, 3, 4, 5, 6, 7) for f in listed)
    assert not any(int(row[0]) in (9, 10) for row in lstm.get_tensor("kernel_form_list").reshape(-1, 5)), "a BiLSTM handle lists what it listed"
    after = [a.numpy() for a in lstm.beam_search_prediction((world["raw"], world["ev"]), 5, WORLD.L)]
    assert np.array_equal(after[0], before[0]) and np.array_equal(_bits(after[1]), _bits(before[1]))
    lstm.close()
    import ctypes
    ccfg, h = bc.cfg.to_c(), ctypes.c_void_p()
    assert bc._lib.rv_create_rnn(ctypes.byref(ccfg), 2, ctypes.byref(h)) == -5 and not h, "a family that is not built: RV_EUNSUPPORTED, no handle"


# ---------------------------------------------------------------------------------------------- windows that do not fit in LDS
def _gru_lds_bytes(F, T):
    """gru_lds_bytes of csrc/gru_mx.hip, restated: the h image (16 KB), 384 factors and 384 recurrent biases, and for a layer-0 form
    (F > 0) its F + 1 rows of 384 input weights / biases and the sixteen chunks' windows of T steps x F features, as floats."""
    return 16384 + 4 * (2 * 384 + ((F + 1) * 384 + 16 * T * F if F > 0 else 0))


LDS_LIMIT = 160 * 1024
DECODE_STEPS = 352                  # the attention memory the decode kernels are built for


def _last_fit(F):
    return max(T for T in range(1, 1 << 14) if _gru_lds_bytes(F, T) <= LDS_LIMIT)


def test_windows_beyond_the_lds_are_refused_and_the_last_that_fit_work(rv):
    """rv_create_rnn on both sides of each LDS edge of k_gru_rec_mx's layer-0 forms: the first max_event_len / max_raw_len that does not
    fit is RV_EUNSUPPORTED by name, with no handle; the last that fits gives a handle that works at the decode's 352 steps, returns the
    bytes of a handle sized to the call, refuses T_m = 353 by name and works on.  (The case names lds-event-T115 / T116 are the two sides
    of 64 KB by the same formula.)"""
    import ctypes
    te, tr = _last_fit(5), _last_fit(1)
    assert _gru_lds_bytes(5, te) <= LDS_LIMIT < _gru_lds_bytes(5, te + 1) and (te, tr) == (422, 2208)
    assert _gru_lds_bytes(1, tr) == LDS_LIMIT < _gru_lds_bytes(1, tr + 1), "2208 samples take the 160 KB exactly"
    assert _gru_lds_bytes(5, 115) < 64 * 1024 < _gru_lds_bytes(5, 116) and _gru_lds_bytes(5, DECODE_STEPS) == 141312
    lib = rv._capi.load_library()
    for mode, key, T in (("event", "max_event_len", te + 1), ("joint", "max_event_len", te + 1), ("raw", "max_raw_len", tr + 1),
                         ("joint", "max_raw_len", tr + 1)):
        cfg = rv.config.RvConfig(mode=mode, rnn="bigru", max_batch=2, **{key: T})
        ccfg, h = cfg.to_c(), ctypes.c_void_p()
        rc = lib.rv_create_rnn(ctypes.byref(ccfg), 1, ctypes.byref(h))
        msg = (lib.rv_last_error(None) or b"").decode()
        assert rc == -5 and not h, (mode, key, T, rc)
        assert "bigru" in msg and key in msg and str(T) in msg and "160 KB" in msg, (mode, key, msg)
    # the longest raw window that fits: a handle, and a call at the decode's limit on it
    long_raw = C.BY_NAME["long-raw-T352"]
    r = C.fp64(rv, long_raw.name)
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "raw", 0.0, encoder_depth=long_raw.enc_depth, rnn_type="bigru", max_batch=2,
                       max_raw_len=tr, max_output_len=long_raw.L)
    bc.set_weights_flat(C.weights(rv, long_raw.enc_depth, 1, "raw", "luong")[0])
    assert long_raw.Tr == DECODE_STEPS
    tok, lg = (a.numpy() for a in bc.greedy_search_prediction(r["raw"][:2], long_raw.L))
    (og, olg), o = C.sliced(r["out"], r["taps"], [0, 1])
    e, _ = _greedy_errors(tok, lg, None, og, olg, o)
    print(f"max_raw_len {tr}, T_r {DECODE_STEPS}: step logits {e['step_logits']:.2e} from fp64")
    assert tok.shape[0] == 2 and e["step_logits"] < TOL
    bc.close()
    # the longest event window that fits: the bytes of the handle sized to the call; 353 steps refused by name; the next call right
    c = C.BY_NAME["lds-event-T352"]
    r = C.fp64(rv, c.name)
    assert c.Te == DECODE_STEPS and c.mode == "event"
    sized = _open(rv, c)
    want = [a.numpy().copy() for a in sized.beam_search_prediction(r["ev"], c.W, c.L)]
    sized.close()
    big = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "event", 0.0, encoder_depth=c.enc_depth, rnn_type="bigru", max_batch=c.B,
                        max_event_len=te, max_output_len=c.L, max_beam=c.W)
    big.set_weights_flat(C.weights(rv, c.enc_depth, c.dec_depth, c.mode, c.attention)[0])
    for again in range(2):
        got = [a.numpy() for a in big.beam_search_prediction(r["ev"], c.W, c.L)]
        assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])), again
        if again == 0:
            over = np.concatenate([r["ev"], r["ev"][:, :1]], axis=1)
            assert over.shape[1] == DECODE_STEPS + 1 <= te
            with pytest.raises(rv._capi.RavventHipError) as ex:
                big.beam_search_prediction(over, c.W, c.L)
            assert "RV_EUNSUPPORTED" in str(ex.value) and str(DECODE_STEPS) in str(ex.value) and str(DECODE_STEPS + 1) in str(ex.value), str(ex.value)
    big.close()


# ---------------------------------------------------------------------------------------------- adversarial weights
@pytest.mark.parametrize("saturate", [False, True], ids=["plain", "saturated"])
@pytest.mark.parametrize("col_gain", C.ADV_GAINS)
def test_encoder_adversarial_recurrent_kernel(rv, col_gain, saturate):
    """k_gru_rec_mx (F = 1, 5 and 0; both directions, two layers, 150 + 25 steps) on the recipes of gru_cases.adversarial_encoder: in every
    encoder cell's U one row x 30, one row x 1e-5, a z column and two h columns x 8 or x 50; with `saturate` the first 64 units' z gates
    closed and their candidates at +-1, so that half of h sits on the edge the 2^14 image rests on.  The regime is asserted on the
    reference; then enc_output is finite, nowhere beyond 1 in size, within TOL of fp64 and within TWIN_K x the fp32 twin + TWIN_C -- the
    one relative bound: the family has no second recurrence form to compare with.  The keys likewise.  An activation that is accurate
    absolutely but not relatively (tanh as 2 sigmoid(2x) - 1) passes every other GRU case and fails here, as the BiLSTM kernels once did."""
    a = C.adversarial_encoder(rv, col_gain, saturate)
    if saturate:
        assert a["saturated"] > 0.3, a["saturated"]
    else:
        assert a["preact"] > 10.0, a["preact"]
    c = C._c("adversarial-enc", C.ADV_B, "joint", C.ADV_TR, C.ADV_TE, enc_depth=2, W=3, L=6)
    bc = _open(rv, c, flat=a["flat"])
    bc.set_option("debug_taps", 1)
    bc.beam_search_prediction((a["raw"], a["ev"]), c.W, c.L)
    Tm = c.Tr + c.Te
    enc = bc.get_tensor("enc_output").reshape(c.B, Tm, 256)
    keys = bc.get_tensor("keys").reshape(c.B, Tm, 128)
    assert (bc.get_tensor("mask").reshape(c.B, Tm) == a["mask"]).all()
    forms = {tuple(int(v) for v in row) for row in bc.get_tensor("kernel_forms").reshape(-1, 5)}
    assert {f for f in forms if f[0] == 9} == {(9, F, 16, 0, 0) for F in (0, 1, 5)}, sorted(forms)
    bc.close()
    assert np.isfinite(enc).all() and np.isfinite(keys).all()
    assert np.abs(enc).max() <= 1.0, float(np.abs(enc).max())
    err = _memory_errors(enc, keys, a)
    tag = f"adversarial encoder gain {col_gain:g} {'saturated' if saturate else 'plain'}"
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e} (twin {a['twin'][k]:.2e})" for k, v in err.items()) + f"; saturated share {a['saturated']:.3f}, pre-activation {a['preact']:.1f}")
    for k, v in err.items():
        assert v < TOL, (tag, k, v, a["twin"][k])
    _assert_twin(err, a["twin"], tag)


@pytest.mark.parametrize("dec_depth", [1, 2])
def test_decoder_cell_adversarial_recurrent_kernel(rv, dec_depth):
    """k_dec_cell_gru, one and two stacked cells, on gru_cases.adversarial_decoder: two h-gate columns of each cell's U x 50, one row x 30,
    one row x 1e-5, the end token suppressed so that all L - 1 steps run.  Step logits and alignments over the steps that agree with the
    fp64 beam within TOL and within TWIN_K x the fp32 twin + TWIN_C; a chunk that leaves the fp64 beam does so through a near-tie, and at
    most B // 4 do (the twin meets that cap: test_gru.py)."""
    a = C.adversarial_decoder(rv, dec_depth)
    c, o, twin = a["case"], a["taps"], a["twin"]
    bc = _open(rv, c, flat=a["flat"])
    bc.set_option("debug_taps", 1)
    tok, sc = (x.numpy() for x in bc.beam_search_prediction((a["raw"], a["ev"]), c.W, c.L))
    S, B, W, Tm = tok.shape[1], c.B, c.W, c.Tr + c.Te
    assert S == c.L - 1 == o["step_ids"].shape[0]
    lgs = bc.get_tensor("step_logits").reshape(S, B, W, 7)
    al = bc.get_tensor("step_alignments").reshape(S, B, W, Tm)
    ids = bc.get_tensor("step_ids").reshape(S, B, W).astype(np.int64)
    par = bc.get_tensor("parent_ids").reshape(S, B, W).astype(np.int64)
    forms = {tuple(int(v) for v in row) for row in bc.get_tensor("kernel_forms").reshape(-1, 5)}
    assert (10, 0, 0, 0, 0) in forms, sorted(forms)
    bc.close()
    assert np.isfinite(lgs).all() and np.isfinite(al).all()
    err, left = _beam_errors(lgs, al, ids, par, np.full(B, S), None, o, a["out"][1])
    for i in left:
        gap = _near_tie_gap(G, o["step_logits"][:, i], W, a["cfg"]["end_token"])
        assert gap < _tie_bound(twin), (c.name, i, "left the fp64 beam with no near-tie", gap)
    assert len(left) <= B // 4, (c.name, "chunks that left the fp64 decode", left)
    print(f"{c.name}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) + f"; chunks that left: {left}")
    for k, v in err.items():
        assert v < TOL, (c.name, k, v)
    _assert_twin(err, twin, c.name)
