"""Coalesced asynchronous calls (option `coalesce`): consecutively submitted slabs decoded as ONE internal call must give every slab the
bytes, the S and the padding of its own synchronous call, whatever way the group came to be launched.

Shapes: those of test_asynchronous_calls_match_synchronous (max_batch 40, T 120 + 20, beam 5, L 24), base-emitting weights with the
end-token bias raised so that chunks -- and therefore slabs -- stop at different steps, and slab sizes chosen so that the 16-chunk
recurrence workgroups straddle members, one member is empty and the chunks of a group are no multiple of 16.  The weight seed and the
bias were picked with the CPU port (oracle/cpu_port.py): it gives S = 17 15 13 13 8 13 0 15 13 18 for the ten slabs, so every group
of 2, 3 or 4 consecutive slabs holds members with different S; the tests assert that from the synchronous results before they rely on it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (40, 7, 33, 40, 1, 17, 0, 25, 40, 12)
T_R, T_E, W, L = 120, 20, 5, 24
STEPS = L - 1


def _flat(rv, cfg):
    flat = rv.weights.init_weights(cfg, seed=7, gain=3.0)
    letters = [t for t in range(cfg.vocab) if t not in (cfg.start_token, cfg.end_token, cfg.pad_token)]
    flat["b_fc"][letters] += 1.5
    flat["b_fc"][cfg.end_token] += 1.5
    return flat


def _handle(rv):
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=2, attention_type="luong",
                       honor_attention_type=True, max_batch=40, max_raw_len=T_R, max_event_len=T_E, max_output_len=L)
    flat = _flat(rv, bc.cfg)
    bc.set_weights_flat(flat)
    return bc, flat


@pytest.fixture(scope="module")
def world(rv):
    """One handle, the ten slabs and their synchronous results (computed once, never modified)."""
    import torch
    bc, flat = _handle(rv)
    slabs = [rv.synthetic.make_slab(n, T_R, T_E, seed=100 + i)[:2] for i, n in enumerate(SIZES)]
    dev = [(torch.from_numpy(r).cuda(), torch.from_numpy(e).cuda()) for r, e in slabs]
    ref = []
    for x in dev:        # the whole [B, L-1] output buffers of the synchronous call: columns >= S hold its padding
        t, s = bc.beam_search_prediction(x, W, L)
        S = int(t.shape[1])
        tf, sf = (t._base if t._base is not None else t), (s._base if s._base is not None else s)
        ref.append((tf.cpu().numpy().copy().reshape(-1, STEPS), sf.cpu().numpy().copy().reshape(-1, STEPS), S))
    ref_calls = [tuple(a.copy() for a in bc.beam_search_call_arrays(x, W, L)) for x in slabs]
    for r in ref:
        r[0].setflags(write=False); r[1].setflags(write=False)
    w = {"bc": bc, "flat": flat, "slabs": slabs, "dev": dev, "ref": ref, "ref_calls": ref_calls, "S": [r[2] for r in ref]}
    yield w
    bc.close()


def _same(got, want):
    """(tokens, scores) as the calls return them ([B, S] views) against the synchronous call's: shape (so S), tokens, score bits."""
    t, s = np.asarray(got[0].cpu() if hasattr(got[0], "cpu") else got[0]), np.asarray(got[1].cpu() if hasattr(got[1], "cpu") else got[1])
    S = want[2]
    return t.shape == (want[0].shape[0], S) and np.array_equal(t, want[0][:, :S]) and np.array_equal(s.view(np.int32), want[1][:, :S].view(np.int32))


def _stats(bc):
    g, n, largest, in_force = bc.get_tensor("coalesce_stats")
    return int(g), int(n), int(largest), int(in_force)


def test_members_of_a_group_stop_at_different_steps(world):
    """The precondition of everything below, from the synchronous results: in every grouping the tests use, some group holds a member
    whose S is the group's maximum and another whose S is not -- a finalize that gave every member the group's S could not pass."""
    S = world["S"]
    print("S per slab:", S)
    assert S[SIZES.index(0)] == 0
    for n in (2, 3, 4):
        groups = [S[i:i + n] for i in range(0, len(S), n)]
        assert any(len(g) >= 2 and min(x for x in g) < max(g) for g in groups), (n, groups)
        assert any(len([x for x in g if x > 0]) >= 2 and len(set(x for x in g if x > 0)) >= 2 for g in groups), (n, groups)


@pytest.mark.parametrize("depth", [4, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_coalesced_slabs_equal_synchronous(world, rv, n, depth):
    import torch
    bc, slabs, dev, ref, ref_calls = (world[k] for k in ("bc", "slabs", "dev", "ref", "ref_calls"))
    bc.set_async_depth(depth)
    bc.set_coalesce(n)
    g0, s0, _, in_force = _stats(bc)
    assert in_force == n
    # host inputs
    outs = list(bc.beam_search_stream(slabs, W, L))
    assert len(outs) == len(slabs) and all(_same(o, r) for o, r in zip(outs, ref))
    g1, s1, largest, _ = _stats(bc)
    if n == 1:
        assert (g1, s1) == (g0, s0), "coalesce 1 must not form groups"
    else:
        assert s1 - s0 == len(slabs) and largest >= n and g1 - g0 == -(-len(slabs) // n), (g0, s0, g1, s1, largest)
    # device inputs, fresh tensors per slab (the library must have taken its copy, or keep reading them, until collect)
    fresh = ((r.clone(), e.clone()) for r, e in dev)
    outs = list(bc.beam_search_stream(fresh, W, L))
    assert all(_same(o, r) for o, r in zip(outs, ref))
    # caller-provided outputs: whole buffers, padding of the columns >= S included
    mine = [(torch.full((b, STEPS), -7, dtype=torch.int32, device="cuda"), torch.full((b, STEPS), -7.0, device="cuda")) for b in SIZES]
    outs = list(bc.beam_search_stream(dev, W, L, outs=mine))
    assert all(_same(o, r) for o, r in zip(outs, ref))
    for (t, s), r, b in zip(mine, ref, SIZES):
        if b:
            assert np.array_equal(t.cpu().numpy(), r[0]) and np.array_equal(s.cpu().numpy().view(np.int32), r[1].view(np.int32))
    # raw output addresses inside one gather buffer
    rows = int(sum(SIZES))
    gt = torch.full((rows, STEPS), -7, dtype=torch.int32, device="cuda")
    gs = torch.full((rows, STEPS), -7.0, device="cuda")
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    queue, got_S = [], []
    for i, x in enumerate(dev):
        if len(queue) >= depth:
            got_S.append(bc.collect(queue.pop(0)))
        queue.append(bc.submit_beam_search(x, W, L, out_ptrs=(gt.data_ptr() + 4 * STEPS * int(offs[i]), gs.data_ptr() + 4 * STEPS * int(offs[i]))))
    while queue:
        got_S.append(bc.collect(queue.pop(0)))
    assert got_S == world["S"]
    gt, gs = gt.cpu().numpy(), gs.cpu().numpy()
    for i, r in enumerate(ref):
        assert np.array_equal(gt[offs[i]:offs[i + 1]], r[0]) and np.array_equal(gs[offs[i]:offs[i + 1]].view(np.int32), r[1].view(np.int32)), i
    # fused post-processing
    for got, want in zip(bc.beam_search_stream(slabs, W, L, calls=True), ref_calls):
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert bc.last_steps == world["S"][-1]


def test_every_event_that_launches_a_group_early(world, rv):
    bc, slabs, dev, ref, flat = (world[k] for k in ("bc", "slabs", "dev", "ref", "flat"))
    bc.set_async_depth(6)
    bc.set_coalesce(3)
    launched = lambda: _stats(bc)[0]
    # a ticket of a group that has not filled: its first member, then (another group) its last member
    g0 = launched()
    t = [bc.submit_beam_search(dev[i], W, L) for i in (0, 1)]
    assert launched() == g0
    assert _same(bc.collect(t[0]), ref[0]) and launched() == g0 + 1
    assert _same(bc.collect(t[1]), ref[1])
    t = [bc.submit_beam_search(slabs[i], W, L) for i in (2, 3)]
    assert _same(bc.collect(t[1]), ref[3]) and launched() == g0 + 2
    assert _same(bc.collect(t[0]), ref[2])
    # two full groups, collected in reverse; the seventh slab is refused
    t = [bc.submit_beam_search(dev[i], W, L) for i in range(4, 10)]
    assert launched() == g0 + 4
    with pytest.raises(rv._capi.RavventHipError, match="uncollected"):
        bc.submit_beam_search(dev[0], W, L)
    with pytest.raises(rv._capi.RavventHipError, match="in flight"):
        bc.set_weights_flat(flat)
    with pytest.raises(rv._capi.RavventHipError, match="every slab context"):     # async_depth tickets out: no synchronous call either
        bc.beam_search_prediction(dev[0], W, L)
    for i in reversed(range(6)):
        assert _same(bc.collect(t[i]), ref[4 + i]), i
    with pytest.raises(rv._capi.RavventHipError):
        bc.collect(t[0])
    # a slab with another T_e in the middle of a group: the group goes as it is, the odd slab alone
    odd = (slabs[1][0], np.ascontiguousarray(slabs[1][1][:, :12]))
    to, so = bc.beam_search_prediction(odd, W, L)
    g1 = launched()
    t = [bc.submit_beam_search(slabs[0], W, L), bc.submit_beam_search(slabs[1], W, L), bc.submit_beam_search(odd, W, L),
         bc.submit_beam_search(slabs[2], W, L)]
    assert launched() == g1 + 2          # (0, 1) when the odd slab came, the odd slab when slab 2 came
    got = [bc.collect(x) for x in t]
    assert launched() == g1 + 3
    assert _same(got[0], ref[0]) and _same(got[1], ref[1]) and _same(got[3], ref[2])
    assert got[2][0].shape == to.shape and np.array_equal(got[2][0].numpy(), to.numpy()) and np.array_equal(got[2][1].numpy(), so.numpy())
    # a synchronous call while a group is filling
    g2 = launched()
    t = [bc.submit_beam_search(dev[i], W, L) for i in (7, 8)]
    mid = bc.beam_search_prediction(dev[9], W, L)
    assert launched() == g2 + 1 and _same(mid, ref[9])
    assert _same(bc.collect(t[0]), ref[7]) and _same(bc.collect(t[1]), ref[8])
    # rv_beam_search_flush; nothing to do without a group
    bc.flush()
    assert launched() == g2 + 1
    t = bc.submit_beam_search(dev[5], W, L)
    bc.flush()
    assert launched() == g2 + 2
    # set_option launches the group (it was submitted under the old options); weights stay refused while tickets are out
    t2 = bc.submit_beam_search(dev[3], W, L)
    bc.set_option("attend_threads", 0)
    assert launched() == g2 + 3
    t3 = bc.submit_beam_search(dev[4], W, L)
    with pytest.raises(rv._capi.RavventHipError, match="in flight"):
        bc.set_weights_flat(flat)
    assert launched() == g2 + 4
    assert _same(bc.collect(t3), ref[4]) and _same(bc.collect(t), ref[5]) and _same(bc.collect(t2), ref[3])
    bc.set_weights_flat(flat)            # nothing in flight: accepted
    assert _same(next(iter(bc.beam_search_stream(dev[:1], W, L))), ref[0])


def test_close_with_a_launched_and_an_unlaunched_group(world, rv):
    bc, _ = _handle(rv)
    bc.set_async_depth(6)
    bc.set_coalesce(3)
    t = [bc.submit_beam_search(world["dev"][i], W, L) for i in range(3)] + [bc.submit_beam_search(world["slabs"][3], W, L)]
    assert _stats(bc)[:3] == (1, 3, 3)
    assert _same(bc.collect(t[1]), world["ref"][1])
    bc.close()


def test_what_is_never_coalesced(world, rv):
    bc, slabs, dev, ref = (world[k] for k in ("bc", "slabs", "dev", "ref"))
    bc.set_coalesce(-1)
    bc.set_async_depth(2)                # the default rule: a caller with up to three slabs in flight never has one held back
    assert _stats(bc)[3] == 1
    bc.set_async_depth(3)
    assert _stats(bc)[3] == 1
    g0 = _stats(bc)[:2]
    outs = list(bc.beam_search_stream(dev, W, L))
    assert all(_same(o, r) for o, r in zip(outs, ref)) and _stats(bc)[:2] == g0
    for d in range(4, 17):               # ... and beyond that never more than half the depth
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bc.set_async_depth(d)
        assert 1 <= _stats(bc)[3] <= d // 2
    bc.set_async_depth(6)
    bc.set_coalesce(3)
    # greedy search (its stopping rule is slab-wide) and the tapped decode run as they always did
    bc.greedy_search_prediction(dev[1], L)
    assert _stats(bc)[:2] == g0
    bc.set_option("persist_taps", 1)
    outs = list(bc.beam_search_stream(dev[:4], W, L))
    bc.set_option("persist_taps", 0)
    assert all(_same(o, r) for o, r in zip(outs, ref)) and _stats(bc)[:2] == g0
    bc.set_option("profile", 1)
    outs = list(bc.beam_search_stream(dev[:4], W, L))
    bc.set_option("profile", 0)
    assert all(_same(o, r) for o, r in zip(outs, ref)) and _stats(bc)[:2] == g0
    outs = list(bc.beam_search_stream(dev[:4], W, L))
    assert all(_same(o, r) for o, r in zip(outs, ref)) and _stats(bc)[1] == g0[1] + 4


def test_call_kinds_do_not_leak_into_the_next_call(world, rv):
    """Every kind of call through the same contexts, one after the other: what one kind adds to a call (the whole beam, forced
    labels, a letter table, a member table) must be gone when the next call is recorded, so every plain beam search between them
    gives the bytes of the fixture's synchronous reference."""
    bc, dev, ref = (world[k] for k in ("bc", "dev", "ref"))
    big, small = SIZES.index(7), SIZES.index(1)
    x, want = dev[big], ref[big]
    cfg = bc.cfg
    plain = lambda: _same(bc.beam_search_prediction(x, W, L), want)
    slot0 = lambda hyp: _same((hyp.tokens[:, :, 0], hyp.scores[:, :, 0]), want)
    fresh, _ = _handle(rv)
    greedy_want = [a.cpu().numpy().copy() for a in fresh.greedy_search_prediction(x, L)]
    fresh.close()
    bc.set_coalesce(-1)
    bc.set_async_depth(4)
    try:
        assert plain()                                                       # 1
        assert slot0(bc.beam_search_hypotheses(x, W, L))                     # 2
        assert plain()                                                       # 3
        labels = np.full((7, L), cfg.pad_token, np.int32)                    # 4: the plain call's own best tokens as labels
        labels[:, 0] = cfg.start_token
        labels[:, 1:1 + want[2]] = want[0][:, :want[2]]
        sid, logits = bc.teacher_forced_prediction(x, labels)
        assert tuple(sid.shape) == (7, STEPS) and tuple(logits.shape) == (7, STEPS, cfg.vocab)
        greedy = [a.cpu().numpy() for a in bc.greedy_search_prediction(x, L)]                     # 5
        assert greedy[0].shape == greedy_want[0].shape and np.array_equal(greedy[0], greedy_want[0])
        assert np.array_equal(greedy[1].view(np.int32), greedy_want[1].view(np.int32))
        got = bc.beam_search_call_arrays(world["slabs"][big], W, L)          # 6
        assert all(np.array_equal(g, w) for g, w in zip(got, world["ref_calls"][big]))
        assert plain()                                                       # 7
        with pytest.raises(rv._capi.RavventHipError, match="beam width %d outside" % (cfg.max_beam + 1)):       # 8
            bc.beam_search_hypotheses(x, cfg.max_beam + 1, L)
        assert plain()                                                       # 9: the refused call left the handle usable
        bc.set_coalesce(2)                                                   # 10
        g0 = _stats(bc)[0]
        t = [bc.submit_beam_search(dev[big], W, L), bc.submit_beam_search(dev[small], W, L)]
        assert _stats(bc)[0] == g0 + 1
        assert _same(bc.collect(t[0]), ref[big]) and _same(bc.collect(t[1]), ref[small])
        assert slot0(bc.collect(bc.submit_beam_search(x, W, L, all_beams=True)))                  # 11
        assert _same(bc.collect(bc.submit_beam_search(x, W, L)), want)       # 12
        assert plain()                                                       # 13
    finally:
        bc.set_coalesce(-1)
        bc.set_async_depth(2)
