"""The persistent GRU decode on the GPU: option gru_persistent 1 on a bigru handle of one decoder cell, k_dec_persist_gru<W, NIT, ATT>
(kernel id 11), against the numpy reference of tests/gru_reference.py in fp64 and its fp32 twin.

  cases       every form of the list at least once (tests/gru_persist_cases.py: beam 1..8 and greedy, Luong and Bahdanau, T_m = 57, 230,
              352 and 2, seventeen chunks with padded rows, an all-padding chunk under beam and greedy search).  persist_taps 1: step
              logits, alignments and scores within TOL of fp64 and within TWIN_K x the twin + TWIN_C; tokens equal fp64's but at a
              near-tie narrower than _tie_bound, on at most a quarter of a case's kept chunks; the launch is (11, W, NIT, 1, ATT) and no
              k_dec_cell_gru (10) runs.  The measured errors are printed before they are asserted;
  adversarial gru_cases.adversarial_decoder(rv, 1) through the persistent form, the same bounds;
  interfaces  under the option, on the `world` slab of tests/test_gru_gpu.py: the synchronous call against fp64, and bit for bit with it
              the asynchronous calls, a window call (still behind k_expand_windows) and use_graph 0 / 1; all beams and lengths, the
              forced decode's logits and nll_sum, the moves; basecall of a short read;
  beside      option 0 after 1 gives the per-step bytes the `world` fixture recorded before the option was ever set; a BiLSTM handle
              keeps its bytes and its form list; the refusals answer by name and the handle works on.
Measured on one MI355X: step logits 5.5e-07 (2.04e-06 on the adversarial decoder, twin 1.80e-06), alignments
1.96e-07, scores 1.41e-06; no chunk left the fp64 decode.
Without the feature the option key is unknown and id 11 is listed nowhere: every test here fails."""
import numpy as np
import pytest

import gru_cases as C
import gru_persist_cases as P
import gru_reference as G
import test_gru_gpu as T
from test_bench_config_gpu import TWIN_C, TWIN_K  # noqa: F401  (the bounds _assert_twin applies)
from test_gru_gpu import world  # noqa: F401  (the fixture: one per-step handle and its recorded bytes)
from test_parity_gpu import TOL, _assert_twin, _beam_errors, _greedy_errors, _near_tie_gap

pytestmark = pytest.mark.gpu
KID = 11


def _forms(bc, name="kernel_forms"):
    return {tuple(int(v) for v in row) for row in bc.get_tensor(name).reshape(-1, 5)}


def _assert_persistent(bc, want=None):
    """The last synchronous call ran one k_dec_persist_gru form (`want`, if given) and no per-step GRU cell."""
    forms = _forms(bc)
    ran = {f for f in forms if f[0] == KID}
    assert len(ran) == 1 and (want is None or ran == {want}), (want, sorted(forms))
    assert not any(f[0] in (0, 8, 10) for f in forms), ("a per-step cell or an LSTM decode ran", sorted(forms))


def _open(rv, c, **kw):
    bc = T._open(rv, c, **kw)
    bc.set_gru_persistent(True)
    assert bc.gru_persistent
    bc.set_option("persist_taps", 1)
    return bc


def _decode_case(rv, c, r, twin, bc, tag):
    """One case through the persistent form: errors printed, then held to TOL and to the twin; chunks that left fp64 only by a near-tie."""
    keep = C.keep_rows(c)
    o_out, o = C.sliced(r["out"], r["taps"], keep)
    B, Tm = c.B, r["taps"]["mask"].shape[1]
    x = T._x(c.mode, r["raw"], r["ev"])
    if c.W == 0:
        tok, lg = (a.numpy() for a in bc.greedy_search_prediction(x, c.L))
        _assert_persistent(bc, P.form(c))
        S = tok.shape[1]
        al = bc.get_tensor("step_alignments").reshape(S, B, 1, Tm)[:, :, 0]
        og, olg = o_out
        err, left = _greedy_errors(tok[keep], lg[keep], al[:, keep], og, olg, o)
        for i in left:
            s = int(np.nonzero(tok[keep][i, :S] != og[i, :S])[0][0])
            top2 = np.sort(olg[i, s])[-2:]
            assert top2[1] - top2[0] < T._tie_bound(twin), (tag, keep[i], s, "a greedy token differs with no near-tie", float(top2[1] - top2[0]))
        if not left:
            assert S == r["out"][0].shape[1], (tag, S)
        if c.all_pad is not None:
            assert np.isnan(lg[c.all_pad]).all() and np.isnan(al[:, c.all_pad]).all() and (tok[c.all_pad] == 0).all(), tag
    else:
        W, V = c.W, 7
        tok, sc = (a.numpy() for a in bc.beam_search_prediction(x, W, c.L))
        _assert_persistent(bc, P.form(c))
        S = tok.shape[1]
        cs = bc.get_tensor("chunk_steps").astype(int)
        lgs = bc.get_tensor("step_logits").reshape(S, B, W, V)
        al = bc.get_tensor("step_alignments").reshape(S, B, W, Tm)
        ids = bc.get_tensor("step_ids").reshape(S, B, W).astype(np.int64)
        par = bc.get_tensor("parent_ids").reshape(S, B, W).astype(np.int64)
        otok, osc = o_out
        err, left = _beam_errors(lgs[:, keep], al[:, keep], ids[:, keep], par[:, keep], cs[keep], sc[keep], o, osc)
        for i in left:
            gap = _near_tie_gap(G, o["step_logits"][:, i], W, r["cfg"]["end_token"])
            assert gap < T._tie_bound(twin), (tag, keep[i], "left the fp64 beam with no near-tie", gap)
        n = min(S, otok.shape[1])
        for i in (i for i in range(len(keep)) if i not in left):
            assert (tok[keep[i], :n] == otok[i, :n]).all(), (tag, keep[i], "tokens")
        if not left:
            assert S == r["out"][0].shape[1], (tag, S)
        if c.all_pad is not None:
            assert np.isnan(sc[c.all_pad]).all() and (tok[c.all_pad] == 0).all() and np.isnan(al[:, c.all_pad]).all(), tag
            assert np.array_equal(np.isnan(sc), np.isnan(r["out"][1])), tag
    assert len(left) <= len(keep) // 4, (tag, "chunks that left the fp64 decode", left)
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) + f"; chunks that left the fp64 decode: {[keep[i] for i in left]}")
    for k, v in err.items():
        assert v < TOL, (tag, k, v)
    _assert_twin(err, twin, tag)


@pytest.mark.parametrize("name", list(P.BY_NAME))
def test_case_through_the_persistent_form(rv, name):
    c = P.BY_NAME[name]
    bc = _open(rv, c)
    try:
        _decode_case(rv, c, P.fp64(rv, name), P.twin_errors(rv, name), bc, name)
    finally:
        bc.close()


def test_every_listed_form_has_a_case(rv):
    """The forms come from the library's own list: one that is added there without a case here fails."""
    bc = T._open(rv, C.WORLD)
    listed = {f for f in _forms(bc, "kernel_form_list") if f[0] == KID}
    bc.close()
    covered = {P.form(c) for c in P.BY_NAME.values()}
    assert len(listed) == 48 and listed == covered, (sorted(listed - covered), sorted(covered - listed))


def test_adversarial_decoder_through_the_persistent_form(rv):
    a = C.adversarial_decoder(rv, 1)
    c, o, twin = a["case"], a["taps"], a["twin"]
    bc = _open(rv, c, flat=a["flat"])
    tok, sc = (x.numpy() for x in bc.beam_search_prediction((a["raw"], a["ev"]), c.W, c.L))
    _assert_persistent(bc, P.form(c))
    S, B, W, Tm = tok.shape[1], c.B, c.W, c.Tr + c.Te
    assert S == c.L - 1 == o["step_ids"].shape[0]
    cs = bc.get_tensor("chunk_steps").astype(int)
    lgs = bc.get_tensor("step_logits").reshape(S, B, W, 7)
    al = bc.get_tensor("step_alignments").reshape(S, B, W, Tm)
    ids = bc.get_tensor("step_ids").reshape(S, B, W).astype(np.int64)
    par = bc.get_tensor("parent_ids").reshape(S, B, W).astype(np.int64)
    bc.close()
    assert (cs == S).all() and np.isfinite(lgs).all() and np.isfinite(al).all()
    err, left = _beam_errors(lgs, al, ids, par, cs, None, o, a["out"][1])
    for i in left:
        gap = _near_tie_gap(G, o["step_logits"][:, i], W, a["cfg"]["end_token"])
        assert gap < T._tie_bound(twin), (c.name, i, "left the fp64 beam with no near-tie", gap)
    assert len(left) <= B // 4, (c.name, "chunks that left the fp64 decode", left)
    print(f"{c.name} (persistent): " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) + f"; chunks that left: {left}")
    for k, v in err.items():
        assert v < TOL, (c.name, k, v)
    _assert_twin(err, twin, c.name)


# ---------------------------------------------------------------------------------------------- the outer interfaces under the option
@pytest.fixture(scope="module")
def pworld(world):  # noqa: F811
    """The `world` handle with gru_persistent 1 and the synchronous beam search of width 5 under it; the option is 0 again afterwards."""
    bc = world["bc"]
    bc.set_gru_persistent(True)
    tok, sc = (a.numpy().copy() for a in bc.beam_search_prediction((world["raw"], world["ev"]), 5, T.WORLD.L))
    _assert_persistent(bc, (KID, 5, 2, 1, 3))
    for a in (tok, sc):
        a.setflags(write=False)
    yield dict(world, tok=tok, sc=sc)
    bc.set_gru_persistent(False)


def test_sync_call_matches_fp64(pworld):
    T.test_sync_call_matches_fp64(pworld)


def test_all_beams_and_lengths(pworld):
    T.test_all_beams(pworld)
    _assert_persistent(pworld["bc"], (KID, 5, 2, 1, 3))


def test_forced_decode_logits_and_nll_sum(rv, pworld):
    T.test_teacher_forced_logits_and_nll(rv, pworld)
    _assert_persistent(pworld["bc"], (KID, 1, 2, 1, 3))


def test_asynchronous_calls_equal_the_synchronous_call(pworld):
    T.test_asynchronous_calls_equal_the_synchronous_call(pworld)      # (and: nothing is coalesced)


def test_window_call_equals_expanded_rows_behind_the_expansion(rv, pworld):
    T.test_window_table_equals_expanded_rows(rv, pworld)              # (and: k_expand_windows ran once more)
    _assert_persistent(pworld["bc"], (KID, 5, 2, 1, 3))


def test_use_graph_0_equals_1(pworld):
    T.test_use_graph_0_equals_1(pworld)
    _assert_persistent(pworld["bc"], (KID, 5, 2, 1, 3))


def test_moves_against_the_reference_alignments(rv, pworld):
    T.test_moves_against_the_reference_alignments(rv, pworld)
    _assert_persistent(pworld["bc"], (KID, 5, 2, 1, 3))


def test_unfused_memory_projection_gives_the_same_bits(pworld):
    """fused_memory 0: the projection runs as k_gemm_mem_split3 in front of the decode, with the prologue's arithmetic."""
    bc = pworld["bc"]
    try:
        bc.set_option("fused_memory", 0)
        tok, sc = (a.numpy().copy() for a in bc.beam_search_prediction((pworld["raw"], pworld["ev"]), 5, T.WORLD.L))
        _assert_persistent(bc, (KID, 5, 2, 1, 3))
    finally:
        bc.set_option("fused_memory", 1)
    assert np.array_equal(tok, pworld["tok"]) and np.array_equal(T._bits(sc), T._bits(pworld["sc"]))


def test_a_clone_carries_the_option(pworld):
    other = pworld["bc"].clone()
    try:
        assert other.gru_persistent
        tok, sc = (a.numpy() for a in other.beam_search_prediction((pworld["raw"], pworld["ev"]), 5, T.WORLD.L))
        _assert_persistent(other, (KID, 5, 2, 1, 3))
        assert np.array_equal(tok, pworld["tok"]) and np.array_equal(T._bits(sc), T._bits(pworld["sc"]))
    finally:
        other.close()


def test_basecall_of_a_short_read(rv):
    dl = rv.data_loader
    c = C._c("basecall", 16, "joint", dl.MAX_RAW_LEN, dl.MAX_EVENT_LEN, enc_depth=2, W=5, L=24)
    flat, _ = C.weights(rv, 2, 1, "joint", "luong")
    flat = {k: v.copy() for k, v in flat.items()}
    flat["b_fc"][3:7] += 1.5                                          # call bases: a string to merge
    bc = T._open(rv, c)
    flat["b_fc"][bc.cfg.end_token] -= 3.0
    bc.set_gru_persistent(True)                                       # (images from the device copy of the weights in force ...)
    bc.set_weights_flat(flat)                                         # (... and again with the load)
    sig, _ = rv.synthetic.make_read(n_bases=60, seed=3)
    res = bc.basecall(sig, chunk_size=16)
    rw = dl.prepare_windows(sig, stride=6)
    raw, ev = rw.expand()
    n = len(rw)
    parts = [bc.beam_search_call_arrays((raw[a:a + 16], ev[a:a + 16]), 5, 24) for a in range(0, n, 16)]
    _assert_persistent(bc)
    seq, probs = rv.merger.Merger().merge_arrays(*[np.concatenate([p[k] for p in parts]) for k in range(3)])
    assert res.chunks_num == n and len(seq) > 10 and res.seq == seq and res.probs.tobytes() == probs.tobytes()
    bc.set_gru_persistent(False)                                      # ... and the per-step decode is back behind the same handle
    bc.beam_search_call_arrays((raw[:16], ev[:16]), 5, 24)
    assert (10, 0, 0, 0, 0) in _forms(bc) and not any(f[0] == KID for f in _forms(bc))
    bc.close()


# ---------------------------------------------------------------------------------------------- nothing else moved
def test_option_0_after_1_returns_the_per_step_bytes(world):  # noqa: F811
    bc = world["bc"]
    bc.set_gru_persistent(True)
    on = [a.numpy().copy() for a in bc.beam_search_prediction((world["raw"], world["ev"]), 5, T.WORLD.L)]
    _assert_persistent(bc, (KID, 5, 2, 1, 3))
    bc.set_gru_persistent(False)
    assert not bc.gru_persistent
    tok, sc = (a.numpy() for a in bc.beam_search_prediction((world["raw"], world["ev"]), 5, T.WORLD.L))
    forms = _forms(bc)
    assert (10, 0, 0, 0, 0) in forms and not any(f[0] == KID for f in forms), sorted(forms)
    assert np.array_equal(tok, world["tok"]) and np.array_equal(T._bits(sc), T._bits(world["sc"]))
    assert on[0].shape == tok.shape and np.abs(on[1] - sc).max() < 2 * TOL


def test_refusals_and_a_bilstm_handle_beside(rv, world):  # noqa: F811
    err = rv._capi.RavventHipError
    lstm = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=2, max_batch=T.WORLD.B, max_raw_len=50,
                         max_event_len=7, max_output_len=T.WORLD.L)
    lstm.init_random_weights(seed=22)
    before = [a.numpy().copy() for a in lstm.beam_search_prediction((world["raw"], world["ev"]), 5, T.WORLD.L)]
    listed = _forms(lstm, "kernel_form_list")
    assert not any(f[0] in (9, 10, KID) for f in listed), "a BiLSTM handle lists what it listed"
    with pytest.raises(err) as e:
        lstm.set_gru_persistent(True)
    assert "RV_EUNSUPPORTED" in str(e.value) and "bilstm" in str(e.value) and not lstm.gru_persistent
    # two decoder cells: refused by name, and the handle decodes per step as before
    c2 = C.BY_NAME["cell-N65-dec2-luong"]
    two = T._open(rv, c2)
    r2 = C.fp64(rv, c2.name)
    want2 = [a.numpy().copy() for a in two.beam_search_prediction((r2["raw"], r2["ev"]), c2.W, c2.L)]
    with pytest.raises(err) as e:
        two.set_gru_persistent(True)
    assert "RV_EUNSUPPORTED" in str(e.value) and "decoder_depth 2" in str(e.value)
    got2 = [a.numpy() for a in two.beam_search_prediction((r2["raw"], r2["ev"]), c2.W, c2.L)]
    assert np.array_equal(got2[0], want2[0]) and np.array_equal(T._bits(got2[1]), T._bits(want2[1])) and (10, 0, 0, 0, 0) in _forms(two)
    two.close()
    # calls in flight: RV_ESTATE, the ticket still collects, the option then sets
    bc = world["bc"]
    bc.set_async_depth(2)
    t = bc.submit_beam_search((world["raw"], world["ev"]), 5, T.WORLD.L)
    with pytest.raises(err) as e:
        bc.set_gru_persistent(True)
    assert "RV_ESTATE" in str(e.value) and "gru_persistent" in str(e.value) and not bc.gru_persistent
    tok, sc = bc.collect(t)
    assert np.array_equal(tok.cpu().numpy(), world["tok"]) and np.array_equal(T._bits(sc.cpu().numpy()), T._bits(world["sc"]))
    with pytest.raises(err) as e:
        bc.set_option("gru_persistent", 2)
    assert "RV_EINVAL" in str(e.value)
    bc.set_gru_persistent(True)
    with pytest.raises(err) as e:
        bc.set_option("slab_graph", 1)
    assert "RV_EUNSUPPORTED" in str(e.value) and "bigru" in str(e.value)
    bc.beam_search_prediction((world["raw"], world["ev"]), 5, T.WORLD.L)
    _assert_persistent(bc, (KID, 5, 2, 1, 3))
    # persistent-decode options that take the call off the form: the per-step decode and its bytes
    for key in ("persistent_decode", "flash_attend", "matrix_attention", "matrix_cell"):
        try:
            bc.set_option(key, 0)
            tok, sc = (a.numpy() for a in bc.beam_search_prediction((world["raw"], world["ev"]), 5, T.WORLD.L))
            assert (10, 0, 0, 0, 0) in _forms(bc) and np.array_equal(tok, world["tok"]), key
            if key != "flash_attend":                                 # (flash_attend 0 is another per-step attend kernel)
                assert np.array_equal(T._bits(sc), T._bits(world["sc"])), key
        finally:
            bc.set_option(key, 1)
    bc.set_gru_persistent(False)
    after = [a.numpy() for a in lstm.beam_search_prediction((world["raw"], world["ev"]), 5, T.WORLD.L)]
    assert np.array_equal(after[0], before[0]) and np.array_equal(T._bits(after[1]), T._bits(before[1]))
    assert _forms(lstm, "kernel_form_list") == listed
    lstm.close()
