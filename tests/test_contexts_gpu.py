"""What a handle owes its slab contexts and groups, whichever of them a call runs on: a failure anywhere is the handle's error and costs
no slot, options are those in force at each submit, a context's profile lands on the handle, debug taps stay with slot 0, a group's
context takes full slabs while a submit is held to max_batch, and a handle closes with work in flight on every slot.

Shapes are the smallest the paths exist at: bilstm, two encoder layers, one decoder cell, joint mode, max_batch 16, 48 samples + 12
events, L = 8 (seven steps).  The synchronous results are computed once and never modified."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_B, T_R, T_E, W, L = 16, 48, 12, 5, 8
STEPS = L - 1
SIZES = (16, 16, 5)


def _handle(rv):
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=2, decoder_depth=1, rnn_type="bilstm",
                       attention_type="luong", max_batch=MAX_B, max_raw_len=T_R, max_event_len=T_E, max_output_len=L)
    flat = rv.weights.init_weights(bc.cfg, seed=7, gain=3.0)
    letters = [t for t in range(bc.cfg.vocab) if t not in (bc.cfg.start_token, bc.cfg.end_token, bc.cfg.pad_token)]
    flat["b_fc"][letters] += 1.5
    bc.set_weights_flat(flat)
    return bc


@pytest.fixture(scope="module")
def world(rv):
    """The slabs (host arrays) and the (tokens, scores) of their synchronous calls on a fresh handle."""
    bc = _handle(rv)
    slabs = [rv.synthetic.make_slab(n, T_R, T_E, seed=300 + i)[:2] for i, n in enumerate(SIZES)]
    ref = []
    for x in slabs:
        t, s = bc.beam_search_prediction(x, W, L)
        ref.append((t.cpu().numpy().copy(), s.cpu().numpy().copy()))
        ref[-1][0].setflags(write=False); ref[-1][1].setflags(write=False)
    bc.close()
    return {"slabs": slabs, "ref": ref}


def _same(got, want):
    t, s = np.asarray(got[0].cpu()), np.asarray(got[1].cpu())
    return t.shape == want[0].shape and np.array_equal(t, want[0]) and np.array_equal(s.view(np.int32), want[1].view(np.int32))


def test_failure_on_another_slot_reaches_the_handle_and_the_slot_stays_usable(world, rv):
    slabs, ref = world["slabs"], world["ref"]
    bc = _handle(rv)
    try:
        bc.set_async_depth(3)
        bc.set_coalesce(0)
        a = bc.submit_beam_search(slabs[0], W, L)                     # slot 0
        wide = bc.cfg.max_beam + 1
        with pytest.raises(rv._capi.RavventHipError, match="beam width %d outside" % wide):
            bc.submit_beam_search(slabs[1], wide, L)                  # refused on slot 1: the text must be the handle's
        b = bc.submit_beam_search(slabs[2], W, L)                     # slot 1 again: the refused call left it idle
        assert (a["ticket"] & 15, b["ticket"] & 15) == (0, 1)
        assert _same(bc.collect(a), ref[0]) and _same(bc.collect(b), ref[2])
    finally:
        bc.close()


def test_options_are_those_at_each_submit_and_a_context_profiles_into_the_handle(world, rv):
    """Per-kernel profiling (profile 2: the only level that brackets dec_cell; like every level it keeps slabs from coalescing)."""
    slabs, ref = world["slabs"], world["ref"]
    bc = _handle(rv)
    try:
        bc.set_async_depth(2)
        bc.set_option("profile", 2)
        bc.reset_profile()
        a = bc.submit_beam_search(slabs[2], W, L)                     # slot 0, the persistent decode
        bc.set_option("persistent_decode", 0)
        b = bc.submit_beam_search(slabs[2], W, L)                     # slot 1, the per-step kernels
        bc.set_option("persistent_decode", 1)                         # (nothing queued reads options any more)
        assert (a["ticket"] & 15, b["ticket"] & 15) == (0, 1)
        ta, tb = bc.collect(a), bc.collect(b)
        assert _same(ta, ref[2]) and tb[0].shape[0] == SIZES[2]
        prof = bc.profile()
        print("profile:", {k: v[1] for k, v in prof.items()})
        assert "dec_persist" in prof and "dec_cell" in prof
        assert prof["dec_persist"][1] == 1
        assert prof["dec_cell"][1] == STEPS * bc.cfg.dec_depth
    finally:
        bc.close()


def test_taps_belong_to_slot_0(world, rv):
    slabs, ref = world["slabs"], world["ref"]
    bc = _handle(rv)
    try:
        bc.set_async_depth(2)
        bc.set_coalesce(0)
        t = [bc.submit_beam_search(slabs[2], W, L), bc.submit_beam_search(slabs[2], W, L)]
        on0 = [c for c in t if c["ticket"] & 15 == 0]
        other = [c for c in t if c["ticket"] & 15 != 0]
        assert len(on0) == 1 and len(other) == 1
        assert _same(bc.collect(other[0]), ref[2])
        bc.set_option("debug_taps", 1)
        with pytest.raises(rv._capi.RavventHipError, match="debug taps need the handle's own context"):
            bc.beam_search_prediction(slabs[2], W, L)
        assert _same(bc.collect(on0[0]), ref[2])
        tk, _ = bc.beam_search_prediction(slabs[2], W, L)      # (the tapped decode runs the per-step kernels)
        S = int(tk.shape[1])
        assert 1 <= S <= STEPS
        logits = bc.get_tensor("step_logits")
        assert logits.size == S * SIZES[2] * W * bc.cfg.vocab and np.isfinite(logits).all()
    finally:
        bc.close()


def test_a_group_takes_full_slabs_and_a_submit_is_held_to_max_batch(world, rv):
    slabs, ref = world["slabs"], world["ref"]
    bc = _handle(rv)
    try:
        bc.set_async_depth(4)
        bc.set_coalesce(2)
        t = [bc.submit_beam_search(slabs[i], W, L) for i in (0, 1)]   # 2 x max_batch chunks in one internal call
        g, n, largest, _ = (int(v) for v in bc.get_tensor("coalesce_stats"))
        assert (g, n, largest) == (1, 2, 2)
        assert _same(bc.collect(t[0]), ref[0]) and _same(bc.collect(t[1]), ref[1])
        big = rv.synthetic.make_slab(MAX_B + 1, T_R, T_E, seed=9)[:2]
        with pytest.raises(rv._capi.RavventHipError, match="B=%d outside" % (MAX_B + 1)):
            bc.submit_beam_search(big, W, L)
    finally:
        bc.close()


def test_close_with_work_in_flight_on_plain_slots(world, rv):
    slabs, ref = world["slabs"], world["ref"]
    bc = _handle(rv)
    bc.set_async_depth(3)
    bc.set_coalesce(0)
    t = [bc.submit_beam_search(slabs[i], W, L) for i in range(3)]
    assert sorted(c["ticket"] & 15 for c in t) == [0, 1, 2]
    bc.close()
    again = _handle(rv)
    try:
        assert _same(again.beam_search_prediction(slabs[2], W, L), ref[2])
    finally:
        again.close()
