"""The memory layouts the C-ABI accepts (T_r + T_e <= 352) beyond the corner the other files test: long event segments, splits
with more events than raw samples, and a raw / event boundary at one sample or exactly on a 32-row group edge.

A  The layer-0 event recurrences stage their chunks' input windows in dynamic LDS: k_lstm_rec_mx<5, CH> takes 30,720 + 320 T_e
   bytes (65,280 at T_e = 108, 65,600 at 109, 143,360 at 352) and k_lstm_rec_tw<8, 5> 20,480 + 160 T_e (65,440 at 281, 65,600 at
   282, 76,800 at 352), so from T_e = 109 / 282 a launch asks for more than the 64 KB a kernel gets without the opt-in of
   configure_mx_kernels / configure_rec_kernels.  Event mode, two encoder layers, both sides of each edge and the longest window.
   (The HIP runtime these tests were written on grants up to the device's 160 KB without the opt-in too: a library built without
   it passes at T_e = 109 and 352.  The cases hold what the kernels compute with windows that long, whoever admits the launch.)
B  Every k_dec_persist family, the per-step attend kernels and the greedy search over B = 6 chunks of test_kernel_forms_gpu._slab
   at the memories of CASES: event and raw mode on the edges of the NIT bands, joint mode with one raw sample, one event, the
   boundary on a row-group edge (32, 64) and T_e > T_r.
D  Coalesced groups in event and in raw mode, where a group's input buffers have one part only.
(C, the moves over the same boundaries, is in test_moves_gpu.)

Every case asserts the kernel forms it ran by name.  The bounds are the project's own: 1e-4 against fp64, test_parity_gpu._assert_twin
against the oracle's numpy fp32 twin, FORM_TOL between two forms on one slab, masks exact.

Seeds of B: weight seed 70 and slab seed 1000 + i for case i.  On the CPU the oracle's fp32 twin stays on the fp64 decode on all six
chunks of every family x case (test_parity_gpu._stays holds with room); _twin_beam asserts it again on every run."""
import numpy as np
import pytest

from test_kernel_forms_gpu import (ATTEND, ENCODER, FLASH, FMA_OPTS, FORM_TOL, INPROJ, MX_OPTS, PERSIST, PERSIST_FAMILIES, REC, REC_MX,
                                   REC_PROJ, REC_TW, TOL, _beam, _check_beam, _check_forms_agree, _check_greedy, _f, _handle,
                                   _interior_padding, _oracle_inputs, _rows, _set, _slab, _x)
from test_parity_gpu import _assert_twin, _twin_beam, _twin_greedy

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- A
def _event_slab(rv, Bn, Te, sample):
    """Bn chunks of Te events: synthetic.make_slab's suffix padding (up to 10 events), test_kernel_forms_gpu._interior_padding's
    single zero feature and -0.0 feature in every fifth chunk from chunk 3 (its raw part works on a dummy), and the last but one
    sampled chunk live at its last step only."""
    _, ev, _ = rv.synthetic.make_slab(Bn, 1, Te, seed=Bn + Te)
    rng = np.random.default_rng(Bn + Te)
    _interior_padding(np.ones((Bn, 65, 1), np.float32), ev, rng)
    ev[sample[-2], :-1] = 0.0
    ev[sample[-2], -1] = rng.standard_normal(5).astype(np.float32) + 3.0      # (no feature of it is 0.0)
    return ev


def _sample(Bn, groups):
    """Chunk 0, the last chunk, and the first and last chunk of a middle workgroup of each form (G chunks per workgroup)."""
    sample = {0, Bn - 1}
    for G in groups:
        g = (Bn + G - 1) // G // 2
        sample |= {g * G, min(g * G + G - 1, Bn - 1)}
    return sorted(sample)


def _event_forms(bt, opts):
    """The encoder forms of an event-mode call with two layers (bt: chunks per workgroup of the packed-FMA kernels)."""
    if opts["wide_recurrence"] == 0:
        l0 = _f(REC_TW, bt, 5) if opts["tail_wave"] and bt >= 2 else _f(REC, bt, 5)
        return {l0, _f(REC_PROJ, bt, opts["split_projection"]) if opts["fused_projection"] else _f(REC, bt, 0)}
    ch = 16 if opts["wide_recurrence"] == 1 else 8
    return {_f(REC_MX, 5, ch), _f(REC_MX, 0, ch)} if opts["lane_projection"] else {_f(INPROJ, 5), _f(REC_MX, 0, ch)}


def _event_recurrences(rv, oracle, Bn, Te, bt, configs):
    """One beam_search_prediction(ev, 1, 2) per configuration on one slab: the forms by name, the mask of all chunks exact,
    enc_output within 1e-4 and the twin bound of fp64 on the sampled chunks, all chunks within FORM_TOL of the first form."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "event", 0.0, encoder_depth=2, max_batch=Bn, max_raw_len=1,
                       max_event_len=Te, max_output_len=2)
    flat = bc.init_random_weights(seed=41)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    sample = _sample(Bn, {bt, 8, 16})
    ev = _event_slab(rv, Bn, Te, sample)
    omask = oracle.input_mask(ev)
    interior = [b for b in sample if (omask[b] == 0).any() and omask[b, np.argmax(omask[b] == 0):].any()]
    assert interior and omask[sample[-2]].sum() == 1 and omask[sample[-2], -1], "the sampled chunks miss a mask pattern"
    o_enc, _ = oracle.encode_input(w, None, ev[sample], "event", 0.0, np.float64)
    t_enc, _ = oracle.encode_input(w, None, ev[sample], "event", 0.0, np.float32)
    twin = dict(enc_output=float(np.abs(t_enc - o_enc).max()))
    ref = None
    for opts in configs:
        tag = f"event B={Bn} T_e={Te} {opts}"
        _set(bc, opts)
        bc.beam_search_prediction(ev, 1, 2)
        forms = {r for r in _rows(bc, "kernel_forms") if r[0] in ENCODER}
        assert forms == _event_forms(bt, opts), (tag, sorted(forms))
        assert (bc.get_tensor("mask").reshape(Bn, Te) == omask).all(), (tag, "mask")
        enc = bc.get_tensor("enc_output").reshape(Bn, Te, 256)
        err = float(np.abs(enc[sample] - o_enc).max())
        assert err < TOL, (tag, "enc_output vs fp64", err)
        _assert_twin(dict(enc_output=err), twin, "recurrence " + tag)
        if ref is None:
            ref = enc
        else:
            d = float(np.abs(enc - ref).max())
            assert d < FORM_TOL, (tag, "enc_output between forms", d)
    bc.close()


@pytest.mark.parametrize("Te", [108, 109, 352])
def test_event_recurrences_across_the_matrix_pipe_lds_edge(rv, oracle, Te):
    """B = 17: a partial last workgroup at 16 and at 8 chunks per workgroup, one chunk per workgroup on the packed-FMA kernels.
    mx_lds_bytes(5, T_e) crosses 64 KB between T_e = 108 and 109: k_lstm_rec_mx<5, 16> and <5, 8> (lane_projection 1) stage windows
    beyond it; k_inproj_small<5> + k_lstm_rec_mx<0, CH> (lane_projection 0) and the packed-FMA kernels k_lstm_rec<1, 5> +
    k_lstm_rec_proj<1, SB> / k_lstm_rec<1, 0> run the same slab."""
    configs = [dict(tail_wave=1, fused_projection=1, split_projection=2, **o) for o in MX_OPTS] + \
              [dict(wide_recurrence=0, lane_projection=1, **o) for o in FMA_OPTS]
    _event_recurrences(rv, oracle, 17, Te, 1, configs)


@pytest.mark.parametrize("Te", [281, 282, 352])
def test_event_recurrences_across_the_tail_wave_lds_edge(rv, oracle, Te):
    """B = 513, the smallest slab pick_rows_per_block gives eight chunks per workgroup (65 workgroups, the last with one chunk):
    tw_lds_bytes(8, 5, T_e) crosses 64 KB between T_e = 281 and 282.  k_lstm_rec_tw<8, 5> with tail_wave 1, k_lstm_rec<8, 5> with
    tail_wave 0; at T_e = 352 the matrix-pipe forms too: 33 and 65 workgroups, each with a one-chunk last workgroup."""
    configs = [dict(wide_recurrence=0, lane_projection=1, **o) for o in FMA_OPTS[:2]]
    if Te == 352:
        configs += [dict(tail_wave=1, fused_projection=1, split_projection=2, wide_recurrence=wide, lane_projection=1) for wide in (1, 2)]
    _event_recurrences(rv, oracle, 513, Te, 8, configs)


# ---------------------------------------------------------------------------------------------- B
B, W, L = 6, 5, 12
# (mode, T_r, T_e, the NIT of the k_dec_persist that serves T_m); case i takes _slab(.., seed=1000 + i)
CASES = [("event", 0, 64, 2), ("event", 0, 65, 8), ("event", 0, 109, 8), ("event", 0, 256, 8), ("event", 0, 257, 11), ("event", 0, 352, 11),
         ("raw", 352, 0, 11),
         ("joint", 1, 63, 2),          # one raw sample
         ("joint", 32, 33, 8),         # the boundary on a row-group edge
         ("joint", 31, 225, 8),
         ("joint", 64, 192, 8),        # the boundary on a row-group edge
         ("joint", 100, 252, 11),
         ("joint", 1, 351, 11),
         ("joint", 176, 176, 11),
         ("joint", 351, 1, 11)]        # one event
PER_STEP_CASES = {5: 11, 7: 2, 9: 11, 12: 11}       # case -> the TB of the k_dec_attend that serves its T_m (64: 2; 256, 352: 11)
GREEDY_CASES = (5, 12)

_HANDLES, _ORACLE = {}, {}


@pytest.fixture(scope="module")
def handles(rv):
    """One handle per (mode, attention, decoder cells, use): the persistent decode and the per-step kernels keep their own, so no
    test depends on the options another one left."""
    def get(mode, attention, D, use):
        key = (mode, attention, D, use)
        if key not in _HANDLES:
            _HANDLES[key] = _handle(rv, mode, attention, D, seed=70, Tr_max=352, Te_max=352, L=L)
        return _HANDLES[key]
    yield get
    for bc, _ in _HANDLES.values():
        bc.close()
    _HANDLES.clear()
    _ORACLE.clear()


def _case(i):
    mode, Tr, Te, nit = CASES[i]
    raw, ev = _slab(mode, Tr, Te, seed=1000 + i)
    return mode, Tr + Te, nit, _x(mode, raw, ev), _oracle_inputs(mode, raw, ev)


def _fp64_beam(oracle, w, cfg, attention, D, i, r_, e_):
    """The fp64 beam search of case i and its fp32 twin's errors: computed once per (attention, cells, case), never modified."""
    key = (attention, D, i, "beam")
    if key not in _ORACLE:
        taps = {}
        otok, osc = oracle.beam_search(w, cfg, r_, e_, W, L, dtype=np.float64, taps=taps)
        _ORACLE[key] = (taps, otok, osc, _twin_beam(oracle, w, cfg, r_, e_, W, L, taps, osc, f"{attention} D={D} case {i}"))
    return _ORACLE[key]


@pytest.mark.parametrize("i", range(len(CASES)))
@pytest.mark.parametrize("fam", list(PERSIST_FAMILIES))
def test_persistent_decode_over_the_memory_split(handles, oracle, fam, i):
    """Every ATT of the family on case i (beam 5, persist_taps 1) against one fp64 pass: the form by name, _check_beam, and the ATT
    forms against each other."""
    attention, D, _, atts = PERSIST_FAMILIES[fam]
    mode, Tm, nit, x, (r_, e_) = _case(i)
    bc, w = handles(mode, attention, D, "persist")
    bc.set_option("persist_taps", 1)
    cfg = bc.cfg.oracle_cfg()
    taps, otok, osc, twin = _fp64_beam(oracle, w, cfg, attention, D, i, r_, e_)
    got = {}
    for att, opts in atts.items():
        tag = f"{fam} {CASES[i][:3]} ATT={att}"
        _set(bc, opts)
        r = _beam(bc, x, W, L, Tm, persist=True)
        assert r["forms"] == {_f(PERSIST, W, nit, D, att)}, (tag, sorted(r["forms"]))
        got[att] = (r, *_check_beam(oracle, r, taps, otok, osc, W, cfg["end_token"], tag, twin))
    ref = next(iter(atts))
    for att in atts:
        if att != ref:
            _check_forms_agree(got[ref], got[att], f"{fam} {CASES[i][:3]} ATT {ref} vs {att}")


@pytest.mark.parametrize("i", list(PER_STEP_CASES))
@pytest.mark.parametrize("kind", ["flash", "luong", "bahdanau"])
def test_per_step_attend_over_the_memory_split(handles, oracle, kind, i):
    """The per-step kernels (persistent_decode 0, debug_taps 1) at beam 5: k_dec_attend_flash<5, 512>, and k_dec_attend<5, TB> for
    Luong (flash_attend 0) and Bahdanau."""
    attention = "bahdanau" if kind == "bahdanau" else "luong"
    mode, Tm, _, x, (r_, e_) = _case(i)
    bc, w = handles(mode, attention, 1, "per_step")
    cfg = bc.cfg.oracle_cfg()
    _set(bc, dict(persistent_decode=0, debug_taps=1))
    _set(bc, dict(flash_attend=1, attend_threads=512) if kind == "flash" else dict(flash_attend=0))
    want = _f(FLASH, W, 512) if kind == "flash" else _f(ATTEND, W, PER_STEP_CASES[i])
    taps, otok, osc, twin = _fp64_beam(oracle, w, cfg, attention, 1, i, r_, e_)
    tag = f"{kind} {CASES[i][:3]}"
    r = _beam(bc, x, W, L, Tm, persist=False)
    assert r["forms"] == {want}, (tag, sorted(r["forms"]))
    _check_beam(oracle, r, taps, otok, osc, W, cfg["end_token"], tag, twin)


@pytest.mark.parametrize("i", GREEDY_CASES)
@pytest.mark.parametrize("fam", [f for f, spec in PERSIST_FAMILIES.items() if spec[1] == 1])
def test_greedy_search_over_the_memory_split(handles, oracle, fam, i):
    """The greedy search of every ATT of the one-cell families on the longest event-mode memory and on 1 + 351."""
    attention, D, _, atts = PERSIST_FAMILIES[fam]
    mode, Tm, nit, x, (r_, e_) = _case(i)
    bc, w = handles(mode, attention, D, "persist")
    bc.set_option("persist_taps", 1)
    cfg = bc.cfg.oracle_cfg()
    gtaps = {}
    og, olg = oracle.greedy_search(w, cfg, r_, e_, L, dtype=np.float64, taps=gtaps)
    gtwin = _twin_greedy(oracle, w, cfg, r_, e_, L, og, olg, gtaps, f"{fam} {CASES[i][:3]} greedy")
    for att, opts in atts.items():
        tag = f"{fam} {CASES[i][:3]} ATT={att} greedy"
        _set(bc, opts)
        assert _check_greedy(bc, x, L, Tm, og, olg, gtaps, tag, gtwin) == {_f(PERSIST, 1, nit, D, att)}, tag


# ---------------------------------------------------------------------------------------------- D
# Coalesced groups with one input part.  Weights: test_coalesce_gpu._flat's scheme (gain 3, base letters + 1.5) with weight seed 7 and
# the end-token bias of CO_END_BIAS, picked with the CPU port (oracle/cpu_port.py; weight seeds 7, 1, 2, 3 x biases 0.5 .. 2.5 tried, most
# of which run every slab to L - 1 or stop all of them after two steps) so that the slabs stop at different steps.  It gives
#   event, T_e = 120, bias 2.0: S = 23 23 15 3 0 19 3 21
#   raw,   T_r = 120, bias 1.0: S = 21 21 21 15 0 22 23 20
# for the eight slabs, so with coalesce 2 and with coalesce 3 some group holds members with different S; the test asserts that from
# the synchronous results before it relies on it.
CO_SIZES = (20, 7, 13, 1, 0, 16, 20, 5)
CO_T, CO_L = 120, 24
CO_STEPS = CO_L - 1
CO_END_BIAS = {"event": 2.0, "raw": 1.0}


def _co_flat(rv, cfg, end_bias):
    flat = rv.weights.init_weights(cfg, seed=7, gain=3.0)
    letters = [t for t in range(cfg.vocab) if t not in (cfg.start_token, cfg.end_token, cfg.pad_token)]
    flat["b_fc"][letters] += 1.5
    flat["b_fc"][cfg.end_token] += end_bias
    return flat


def _co_slabs(rv, mode):
    slabs = [rv.synthetic.make_slab(n, CO_T, CO_T, seed=300 + i)[:2] for i, n in enumerate(CO_SIZES)]
    return [r if mode == "raw" else e for r, e in slabs]


@pytest.fixture(scope="module", params=["event", "raw"])
def world(rv, request):
    """One handle per mode, the eight slabs and their synchronous results (computed once, never modified)."""
    import torch
    mode = request.param
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=2, attention_type="luong",
                       honor_attention_type=True, max_batch=20, max_raw_len=CO_T, max_event_len=CO_T, max_output_len=CO_L)
    bc.set_weights_flat(_co_flat(rv, bc.cfg, CO_END_BIAS[mode]))
    slabs = _co_slabs(rv, mode)
    dev = [torch.from_numpy(x).cuda() for x in slabs]
    ref = []
    for x in dev:        # the whole [B, L-1] output buffers of the synchronous call: columns >= S hold its padding
        t, s = bc.beam_search_prediction(x, W, CO_L)
        S = int(t.shape[1])
        tf, sf = (t._base if t._base is not None else t), (s._base if s._base is not None else s)
        ref.append((tf.cpu().numpy().copy().reshape(-1, CO_STEPS), sf.cpu().numpy().copy().reshape(-1, CO_STEPS), S))
    for r in ref:
        r[0].setflags(write=False); r[1].setflags(write=False)
    ref_calls = [tuple(a.copy() for a in bc.beam_search_call_arrays(x, W, CO_L)) for x in slabs]
    yield dict(mode=mode, bc=bc, slabs=slabs, dev=dev, ref=ref, ref_calls=ref_calls, S=[r[2] for r in ref])
    bc.close()


def test_one_part_slabs_run_the_default_forms(world):
    """The forms behind the synchronous results, by name: a coalesced group runs in a slab context of its own and leaves no form log
    at the handle, so they are read from a synchronous call with persist_taps on (which also keeps the call from replaying a slab
    graph, which has none either); its tokens and score bits are the untapped call's."""
    from test_coalesce_gpu import _same
    bc, dev, ref, mode = (world[k] for k in ("bc", "dev", "ref", "mode"))
    bc.set_option("persist_taps", 1)
    try:
        got = bc.beam_search_prediction(dev[0], W, CO_L)
        forms = _rows(bc, "kernel_forms")
    finally:
        bc.set_option("persist_taps", 0)
    assert forms == {_f(REC_MX, 5 if mode == "event" else 1, 16), _f(REC_MX, 0, 16), _f(PERSIST, W, 8, 1, 3)}, (mode, sorted(forms))
    assert _same(got, ref[0]), mode


@pytest.mark.parametrize("n", [2, 3])
def test_coalesced_slabs_with_one_input_part_equal_synchronous(world, n):
    """test_coalesce_gpu.test_coalesced_slabs_equal_synchronous in event and in raw mode: every slab equals its synchronous call
    in shape (so S), tokens and score bits from host inputs, fresh device inputs and with the fused post-processing, and
    coalesce_stats counts the groups."""
    from test_coalesce_gpu import _same, _stats
    bc, slabs, dev, ref, ref_calls, S = (world[k] for k in ("bc", "slabs", "dev", "ref", "ref_calls", "S"))
    print(f"{world['mode']}: S per slab:", S)
    # the precondition, from the synchronous results: some group holds two non-empty members with different S
    groups = [S[i:i + n] for i in range(0, len(S), n)]
    assert S[CO_SIZES.index(0)] == 0
    assert any(len({x for x in g if x > 0}) >= 2 for g in groups), (n, groups)
    bc.set_async_depth(6)
    bc.set_coalesce(n)
    try:
        g0, s0, _, in_force = _stats(bc)
        assert in_force == n
        # host inputs
        outs = list(bc.beam_search_stream(slabs, W, CO_L))
        assert len(outs) == len(slabs) and all(_same(o, r) for o, r in zip(outs, ref))
        g1, s1, largest, _ = _stats(bc)
        assert s1 - s0 == len(slabs) and largest >= n and g1 - g0 == -(-len(slabs) // n), (g0, s0, g1, s1, largest)
        # device inputs, fresh tensors per slab
        outs = list(bc.beam_search_stream((x.clone() for x in dev), W, CO_L))
        assert all(_same(o, r) for o, r in zip(outs, ref))
        g2, s2, _, _ = _stats(bc)
        assert (g2 - g1, s2 - s1) == (-(-len(slabs) // n), len(slabs)), (g1, s1, g2, s2)
        # fused post-processing
        for got, want in zip(bc.beam_search_stream(slabs, W, CO_L, calls=True), ref_calls):
            assert all(np.array_equal(g, w_) for g, w_ in zip(got, want))
        assert bc.last_steps == S[-1]
    finally:
        bc.set_async_depth(2)
        bc.set_coalesce(-1)
