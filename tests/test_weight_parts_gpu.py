"""Option weight_parts 1 on the GPU: every dense weight rounded to the first f16 part of its image, and the
persistent decode's one-part kernels k_dec_persist_1p, which stream and multiply that part alone.

* the option is accepted and reads back, the one-part forms have a list of their own, "kernel_form_list" is what it was;
* a handle that goes to 1 and back to 2 returns the bytes of one that never left 2;
* in mode 1 the encoder and the attention memory are the fp64 oracle's on weights.rounded_view -- to the fp32 twin's error, which
  the rounding itself exceeds several times over (tests/test_weight_parts.py) -- and step 0 of the decode is within the bound that
  file derives for the rounded output layer;
* one_part_kernels 1 against 0 (the two-part kernels on the images whose second parts are zero): every output identical bit for
  bit but for the sign of a zero, at memory lengths on both edges of every NIT band, through every entry point;
* the forms those cases ran are exactly "kernel_form_list_1p";
* what the mode does not serve is refused by name and leaves the handle as it was.

Slabs, weights (gain 1.5, an end-token bias: chunks finish at different steps) and band edges are tests/test_kernel_forms_gpu.py's."""
import numpy as np
import pytest

from test_kernel_forms_gpu import B, V, _handle, _rows, _slab, _split, _x
from test_parity_gpu import _assert_twin
from test_weight_parts import ENC_CASES, enc_slab, enc_weights, step0, step0_bound

pytestmark = pytest.mark.gpu

L = 10
TMS = (33, 64, 65, 256, 257, 352)          # both edges of the NIT bands 2 (T_m <= 64), 8 (<= 256), 11 (<= 352)
WIDTHS = (1, 5)                            # the widths the one-part list holds (decode.hip: for_each_persist_form_1p)
PERSIST, PERSIST_1P = 0, 8                 # kernel ids of the "kernel_forms" rows (include/ravvent_hip.h)
RAN_1P = set()                             # the one-part forms test_one_part_kernel_is_the_two_part_kernel_bit_for_bit launched


def _nit(Tm):
    return 2 if Tm <= 64 else 8 if Tm <= 256 else 11


def _np(a):
    return a.detach().cpu().numpy().copy() if hasattr(a, "detach") else np.array(a, copy=True)


def _bits(a):
    """Raw bytes, after mapping -0.0 to +0.0 in float arrays (NaN payloads stay)."""
    a = np.ascontiguousarray(_np(a))
    if a.dtype == np.float32:
        a = np.where(a == 0, np.float32(0), a).astype(np.float32)
        return a.view(np.uint32)
    return a


def _same(a, b, what):
    x, y = _bits(a), _bits(b)
    assert x.shape == y.shape, (what, x.shape, y.shape)
    bad = np.argwhere(x != y)
    assert bad.size == 0, f"{what}: {len(bad)} of {x.size} elements differ, first at {bad[:3].tolist()}"


def _persist_rows(bc):
    return {r for r in _rows(bc, "kernel_forms") if r[0] in (PERSIST, PERSIST_1P)}


@pytest.fixture(scope="module")
def world(rv):
    """One joint Luong handle in mode 1 (persist_taps on) with the weights of test_kernel_forms_gpu, and its flat weights."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=2, max_batch=3 * B, max_raw_len=308,
                       max_event_len=90, max_output_len=16)
    flat = rv.weights.init_weights(bc.cfg, seed=70, gain=1.5)
    flat["b_fc"][bc.cfg.end_token] = 0.05
    bc.set_weights_flat(flat)
    bc.set_weight_parts(1)
    bc.set_option("persist_taps", 1)
    yield {"bc": bc, "flat": flat}
    bc.close()


def test_option_is_accepted_and_the_lists_stand(rv):
    bc, _ = _handle(rv, "joint", "luong", 1, seed=70)
    listed = _rows(bc, "kernel_form_list")
    assert bc.weight_parts == 2
    bc.set_option("weight_parts", 1)
    assert bc.weight_parts == 1
    one = _rows(bc, "kernel_form_list_1p")
    assert one == {(PERSIST_1P, W, nit, 1, 3) for W in WIDTHS for nit in (2, 8, 11)}
    assert _rows(bc, "kernel_form_list") == listed and not any(r[0] == PERSIST_1P for r in listed)
    for bad in (0, 3, -1):
        with pytest.raises(rv._capi.RavventHipError, match="weight_parts"):
            bc.set_option("weight_parts", bad)
    assert bc.weight_parts == 1
    with pytest.raises(rv._capi.RavventHipError, match="one_part_kernels"):
        bc.set_option("one_part_kernels", 2)
    # the option is set, the weights in force are still those loaded in mode 2: a clone computes what its source computes
    raw, ev = _slab("joint", 56, 8, seed=5)
    assert bc.weight_parts_loaded == 2
    want = bc.beam_search_prediction((raw, ev), 5, L)
    assert not any(r[0] == PERSIST_1P for r in _rows(bc, "kernel_forms"))
    c = bc.clone()
    assert c.weight_parts == 1 and c.weight_parts_loaded == 2
    got = c.beam_search_prediction((raw, ev), 5, L)
    assert _np(got[0]).tobytes() == _np(want[0]).tobytes() and _np(got[1]).tobytes() == _np(want[1]).tobytes()
    c.close()
    bc.set_weight_parts(1)
    assert bc.weight_parts_loaded == 1
    c = bc.clone()
    assert c.weight_parts == 1 and c.weight_parts_loaded == 1
    want, got = bc.beam_search_prediction((raw, ev), 5, L), c.beam_search_prediction((raw, ev), 5, L)
    assert _np(got[0]).tobytes() == _np(want[0]).tobytes() and _np(got[1]).tobytes() == _np(want[1]).tobytes()
    assert (PERSIST_1P, 5, 2, 1, 3) in _persist_rows(c)
    c.close()
    bc.close()


def test_default_is_untouched_by_a_visit_to_the_mode(rv):
    raw, ev = _slab("joint", 56, 8, seed=5)
    a, _ = _handle(rv, "joint", "luong", 1, seed=70)
    b, _ = _handle(rv, "joint", "luong", 1, seed=70)
    b.set_weight_parts(1)
    there = b.beam_search_hypotheses((raw, ev), 5, L)
    assert (PERSIST_1P, 5, 2, 1, 3) in _persist_rows(b)
    b.set_weight_parts(2)
    ha, hb = a.beam_search_hypotheses((raw, ev), 5, L), b.beam_search_hypotheses((raw, ev), 5, L)
    for f in ha._fields:
        x, y = _np(getattr(ha, f)), _np(getattr(hb, f))
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f
    assert _rows(a, "kernel_forms") == _rows(b, "kernel_forms") and not any(r[0] == PERSIST_1P for r in _rows(b, "kernel_forms"))
    assert _np(there.path_scores).tobytes() != _np(ha.path_scores).tobytes(), "mode 1 returned the full model's scores: nothing was rounded"
    a.close()
    b.close()


@pytest.mark.parametrize("mode,Tr,Te", ENC_CASES)
def test_encoder_and_memory_are_the_rounded_model(rv, oracle, mode, Tr, Te):
    Bn, Tm = 6, Tr + Te
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=2, max_batch=Bn, max_raw_len=Tr, max_event_len=Te,
                       max_output_len=L)
    flat = enc_weights(rv, bc.cfg)
    bc.set_weights_flat(flat)
    bc.set_weight_parts(1)
    bc.set_option("persist_taps", 1)
    raw, ev = enc_slab(rv, Tr, Te)
    wr = rv.weights.flat_to_nested(bc.cfg, rv.weights.rounded_view(bc.cfg, flat))
    e64, m64 = oracle.encode_input(wr, raw, ev, mode, 0.0, np.float64)
    e32, _ = oracle.encode_input(wr, raw, ev, mode, 0.0, np.float32)
    k64, v64 = oracle.setup_memory(wr, e64, m64, np.float64)
    k32, v32 = oracle.setup_memory(wr, e32, m64, np.float32)
    Ac = np.asarray(wr["W_att"])[128:384]
    u64, u32 = v64 @ Ac.astype(np.float64), v32 @ Ac.astype(np.float32)
    twin = dict(enc_output=float(np.abs(e32 - e64).max()), keys=float(np.abs(k32 - k64).max()), values_image=float(np.abs(u32 - u64).max()))
    for wide in (1, 2):
        for fused in (1, 0):
            bc.set_option("wide_recurrence", wide)
            bc.set_option("fused_memory", fused)
            bc.beam_search_prediction((raw, ev), 5, L)
            assert (PERSIST_1P, 5, _nit(Tm), 1, 3) in _persist_rows(bc)
            enc = bc.get_tensor("enc_output").reshape(Bn, Tm, 256)
            mask = bc.get_tensor("mask").reshape(Bn, Tm)
            pm = bc.get_tensor("projected_memory").reshape(Bn, Tm, 256)
            assert (mask == m64).all()
            live = m64.astype(bool)
            err = dict(enc_output=float(np.abs(enc - e64).max()), keys=float(np.abs(pm[..., :128] - k64)[live].max()),
                       values_image=float(np.abs(pm[..., 128:] - u64)[live].max()))
            assert max(err.values()) < 1e-4, err
            _assert_twin(err, twin, f"weight_parts 1 T_m={Tm} wide_recurrence={wide} fused_memory={fused}")
    bc.close()


@pytest.mark.parametrize("W", WIDTHS)
def test_step0_logits_are_the_rounded_model(rv, oracle, world, W):
    bc, flat = world["bc"], world["flat"]
    raw, ev = enc_slab(rv, 40, 12)
    fr = rv.weights.rounded_view(bc.cfg, flat)
    logits, ctxp, h = step0(oracle, rv.weights.flat_to_nested(bc.cfg, fr), bc.cfg, raw, ev)
    _, bound = step0_bound(fr, ctxp, h)
    bc.set_option("one_part_kernels", 1)
    tok, _ = bc.beam_search_prediction((raw, ev), W, L)
    S = tok.shape[1]
    lg = bc.get_tensor("step_logits").reshape(S, 6, W, V)[0, :, 0]
    diff = np.abs(lg - logits)
    print(f"W={W}: step 0 max |logits - fp64 on rounded_view| {diff.max():.2e}, allowed 1e-4 + {bound.min():.2e}..{bound.max():.2e}")
    assert (diff <= 1e-4 + bound).all(), (diff.max(), bound.max())


def _outputs(rv, bc, x, W, Tm, read):
    """Every output of every entry point on one slab, as {name: array}, and the persistent forms that ran."""
    out, forms = {}, set()
    t = lambda name, *shape: bc.get_tensor(name).reshape(shape or (-1,))

    hyp = bc.beam_search_hypotheses(x, W, L)
    forms |= _persist_rows(bc)
    S = hyp.tokens.shape[1]
    cs = t("chunk_steps").astype(int)
    out.update({f"all.{f}": _np(getattr(hyp, f)) for f in hyp._fields})
    lg, al = t("step_logits", S, B, W, V), t("step_alignments", S, B, W, Tm)
    out["chunk_steps"] = cs
    for b in range(B):                         # (rows past a chunk's own last step are not written)
        out[f"step_logits.{b}"], out[f"step_alignments.{b}"] = lg[:cs[b], b].copy(), al[:cs[b], b].copy()
    tok, sc = bc.beam_search_prediction(x, W, L)
    out["tokens"], out["scores"] = _np(tok), _np(sc)
    hyp2, mv = bc.beam_search_moves(x, W, L)
    forms |= _persist_rows(bc)
    out.update({f"moves.{f}": _np(getattr(mv, f)) for f in mv._fields})
    out.update({f"moves.all.{f}": _np(getattr(hyp2, f)) for f in hyp2._fields})
    bases, probs, lens = bc.beam_search_call_arrays(x, W, L)
    out["calls.bases"], out["calls.probs"], out["calls.lengths"] = _np(bases), _np(probs), _np(lens)
    if W == 1:
        g, glg = bc.greedy_search_prediction(x, L)
        forms |= _persist_rows(bc)
        out["greedy.tokens"], out["greedy.logits"] = _np(g), _np(glg)
        labels = np.random.default_rng(Tm).integers(0, V, (B, L)).astype(np.int32)
        fs = bc._teacher_forced(x, labels, bc._train_omit)      # logits, nll, counts of the forced decode
        forms |= _persist_rows(bc)
        out.update({f"forced.{f}": _np(getattr(fs, f)) for f in fs._fields})
    if read is not None:
        handle, rows, T_r, T_e = read
        wt, ws = bc.beam_search_windows(handle.table(rows), W, L, T_r=T_r, T_e=T_e)
        forms |= _persist_rows(bc)
        out["windows.tokens"], out["windows.scores"] = _np(wt), _np(ws)
    return out, forms


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("Tm", TMS)
def test_one_part_kernel_is_the_two_part_kernel_bit_for_bit(rv, world, Tm, W):
    bc = world["bc"]
    Tr, Te = _split(Tm)
    raw, ev = _slab("joint", Tr, Te, seed=1000 + Tm + W)
    x = _x("joint", raw, ev)
    # the window call: chunk b = samples b .. b + T_r - 1 - b and events b .. of one read, padded to the slab's lengths
    rng = np.random.default_rng(Tm)
    handle = bc.put_read(rng.standard_normal(Tr + 2 * B).astype(np.float32), rng.standard_normal((Te + 2 * B, 5)).astype(np.float32))
    rows = np.array([(b, Tr - b, 2 * b, max(Te - b, 1)) for b in range(B)], np.int32)
    got = {}
    for one in (1, 0):
        bc.set_option("one_part_kernels", one)
        got[one] = _outputs(rv, bc, x, W, Tm, (handle, rows, Tr, Te))
    handle.drop()
    (o1, f1), (o0, f0) = got[1], got[0]
    assert f1 == {(PERSIST_1P, W, _nit(Tm), 1, 3)}, f1
    assert f0 == {(PERSIST, W, _nit(Tm), 1, 3)}, f0
    assert set(o1) == set(o0)
    for k in o1:
        _same(o1[k], o0[k], f"T_m={Tm} W={W} {k}")
    assert o1["all.tokens"].shape[1] >= 2 and (o1["chunk_steps"] >= 1).all()
    assert np.isfinite(o1["step_logits.0"]).all() and np.abs(o1["step_logits.0"]).max() > 1e-3
    RAN_1P.update(f1)


@pytest.mark.parametrize("mode,Tr,Te,W", [("raw", 300, 0, 5), ("raw", 64, 0, 1), ("event", 0, 90, 5), ("event", 0, 33, 1)],
                         ids=["raw-Tm300-W5", "raw-Tm64-W1", "event-Tm90-W5", "event-Tm33-W1"])
def test_raw_and_event_modes(rv, oracle, mode, Tr, Te, W):
    """The two one-encoder input modes in mode 1: enc_output is the fp64 oracle's on rounded_view weights (to the fp32 twin), and the
    one-part kernel returns what the two-part kernel returns on the zero-lo images, bit for bit."""
    Tm = Tr + Te
    bc, _ = _handle(rv, mode, "luong", 1, seed=71)
    flat = rv.weights.init_weights(bc.cfg, seed=71, gain=1.5)
    flat["b_fc"][bc.cfg.end_token] = 0.05          # (_handle's weights)
    bc.set_weight_parts(1)
    bc.set_option("persist_taps", 1)
    raw, ev = _slab(mode, Tr, Te, seed=300 + Tm)
    x = _x(mode, raw, ev)
    wr = rv.weights.flat_to_nested(bc.cfg, rv.weights.rounded_view(bc.cfg, flat))
    r_, e_ = (raw if mode == "raw" else None), (ev if mode == "event" else None)
    e64, m64 = oracle.encode_input(wr, r_, e_, mode, 0.0, np.float64)
    e32, _ = oracle.encode_input(wr, r_, e_, mode, 0.0, np.float32)
    got = {}
    for one in (1, 0):
        bc.set_option("one_part_kernels", one)
        hyp = bc.beam_search_hypotheses(x, W, L)
        assert _persist_rows(bc) == {(PERSIST_1P if one else PERSIST, W, _nit(Tm), 1, 3)}
        S = hyp.tokens.shape[1]
        cs = bc.get_tensor("chunk_steps").astype(int)
        lg = bc.get_tensor("step_logits").reshape(S, B, W, V)
        got[one] = {f: _np(getattr(hyp, f)) for f in hyp._fields}
        got[one].update({f"step_logits.{b}": lg[:cs[b], b].copy() for b in range(B)}, chunk_steps=cs)
        enc = bc.get_tensor("enc_output").reshape(B, Tm, 256)
        assert (bc.get_tensor("mask").reshape(B, Tm) == m64).all()
        err = dict(enc_output=float(np.abs(enc - e64).max()))
        assert err["enc_output"] < 1e-4
        _assert_twin(err, dict(enc_output=float(np.abs(e32 - e64).max())), f"weight_parts 1 {mode} T_m={Tm} one_part_kernels={one}")
    for k in got[1]:
        _same(got[1][k], got[0][k], f"{mode} T_m={Tm} W={W} {k}")
    bc.close()


def test_coalesced_group_with_a_member_that_stops_early(rv, world):
    """Three slabs submitted as one coalesced group (one launch of the decode over all their chunks), the middle one a single chunk
    that finishes before the others: every member's results with one_part_kernels 1 equal those with 0, and the synchronous call's."""
    bc = world["bc"]
    W, Tr, Te = 5, 56, 8
    slabs = [_slab("joint", Tr, Te, seed=40), None, _slab("joint", Tr, Te, seed=41)]
    bc.set_option("one_part_kernels", 1)
    sync, steps = {}, {}
    for s in range(8):                         # the single chunk (of eight candidates) that stops first
        r, e = _slab("joint", Tr, Te, seed=50 + s)
        t, _ = bc.beam_search_prediction((r[:1], e[:1]), W, L)
        steps[s] = t.shape[1]
    s = min(steps, key=steps.get)
    r, e = _slab("joint", Tr, Te, seed=50 + s)
    slabs[1] = (r[:1], e[:1])
    for i, x in enumerate(slabs):
        t, sc = bc.beam_search_prediction(x, W, L)
        sync[i] = (_np(t), _np(sc))
    assert sync[1][0].shape[1] < max(sync[0][0].shape[1], sync[2][0].shape[1]), ("a poor probe: no member stops early", steps)
    bc.set_option("persist_taps", 0)           # (a handle with taps on coalesces nothing)
    bc.set_async_depth(4)
    bc.set_coalesce(3)
    got = {}
    try:
        for one in (1, 0):
            bc.set_option("one_part_kernels", one)
            g0 = int(bc.get_tensor("coalesce_stats")[0])
            tickets = [bc.submit_beam_search(x, W, L) for x in slabs]
            got[one] = [tuple(_np(a) for a in bc.collect(t)) for t in tickets]
            assert int(bc.get_tensor("coalesce_stats")[0]) == g0 + 1, "the three slabs did not run as one group"
            ran = {r for r in _rows(bc, "group_kernel_forms") if r[0] in (PERSIST, PERSIST_1P)}
            assert ran == {(PERSIST_1P if one else PERSIST, W, 2, 1, 3)}, (one, ran)      # the group's own launch took the switch
    finally:
        bc.set_coalesce(-1)
        bc.set_async_depth(2)
        bc.set_option("one_part_kernels", 1)
        bc.set_option("persist_taps", 1)
    for i in range(3):
        for j, what in enumerate(("tokens", "scores")):
            _same(got[1][i][j], got[0][i][j], f"member {i} {what}")
            _same(got[1][i][j], sync[i][j], f"member {i} {what} against the synchronous call")


def test_every_listed_one_part_form_ran(world):
    """(after the bit-identity cases, which record the one-part forms they launched)"""
    listed = _rows(world["bc"], "kernel_form_list_1p")
    assert RAN_1P, "run with tests/test_weight_parts_gpu.py::test_one_part_kernel_is_the_two_part_kernel_bit_for_bit"
    missing = listed - RAN_1P
    assert not missing, f"listed one-part forms that no case runs: {sorted(missing)}"
    assert RAN_1P <= listed, f"one-part forms ran that the list does not hold: {sorted(RAN_1P - listed)}"


REFUSED = [
    ("persistent_decode 0", "luong", 1, dict(persistent_decode=0)),
    ("flash_attend 0", "luong", 1, dict(flash_attend=0)),
    ("debug_taps 1", "luong", 1, dict(debug_taps=1)),
    ("matrix_cell 0", "luong", 1, dict(matrix_cell=0)),
    ("matrix_attention 0", "luong", 1, dict(matrix_attention=0)),
    ("two decoder cells", "luong", 2, {}),
    ("three decoder cells", "luong", 3, {}),
    ("bahdanau", "bahdanau", 1, {}),
]


@pytest.mark.parametrize("name,attention,D,opts", REFUSED, ids=[r[0] for r in REFUSED])
def test_what_the_mode_does_not_serve_is_refused(rv, name, attention, D, opts):
    bc, _ = _handle(rv, "joint", attention, D, seed=70)
    raw, ev = _slab("joint", 56, 8, seed=5)
    bc.set_weight_parts(1)
    before = None
    if not (D > 1 or attention != "luong"):
        t, s = bc.beam_search_prediction((raw, ev), 5, L)
        before = (_np(t), _np(s))
    for k, v in opts.items():
        bc.set_option(k, v)
    for call in (lambda: bc.beam_search_prediction((raw, ev), 5, L), lambda: bc.greedy_search_prediction((raw, ev), L),
                 lambda: bc.beam_search_hypotheses((raw, ev), 3, L)):
        with pytest.raises(rv._capi.RavventHipError, match="weight_parts") as ei:
            call()
        assert "RV_EUNSUPPORTED" in str(ei.value), str(ei.value)
    for k, v in opts.items():
        bc.set_option(k, 1 - v)
    if before is not None:
        t, s = bc.beam_search_prediction((raw, ev), 5, L)
        assert _np(t).tobytes() == before[0].tobytes() and _np(s).tobytes() == before[1].tobytes()
    else:                                      # the configuration itself is what is refused: back in mode 2 the handle serves the call
        bc.set_weight_parts(2)
        t, _ = bc.beam_search_prediction((raw, ev), 5, L)
        assert t.shape[0] == B
    bc.close()
