"""Beam search over windows of reads that lie on the device once (rv_read_put*, rv_beam_search_windows*).

The reference of every assertion is the library's own chunk-tensor path: the same handle given `data_loader.expand_windows(...)` of
the same rows through rv_beam_search / rv_beam_search_calls.  A window call only changes where a chunk's bytes are read from, so
tokens, score bits, S, the mask and the encoder output must be identical, under every option and on every call path.

Shapes: T_r = 40, T_e = 8, L = 8, two encoder layers, one synthetic read of about 600 samples, hand-made tables of 19 rows -- two
workgroups of the 16-chunk recurrence with three live rows in the second, three of the 8-chunk form.  The rows: a window from sample
0, one that ends on the read's last sample and last event, full-length windows, a zero-length raw window beside a real event window
and the reverse, odd starts, heavy overlap, and a sample that is exactly 0.0 (= the padding value) inside a window, so that the mask
is 0 at a real position."""

import numpy as np
import pytest

from test_coalesce_gpu import _same, _stats
from test_parity_gpu import _emitting_flat

pytestmark = pytest.mark.gpu

T_R, T_E, L, B = 40, 8, 8, 19
ZERO_AT = 7


def _x(mode, raw, ev):
    return {"joint": (raw, ev), "raw": raw, "event": ev}[mode]


def _make_read(rv, seed, n_bases=66):
    """(raw_sc [N], events_sc [E,5]) of a seeded synthetic read, through the chunker's own scaling."""
    sig, _ = rv.synthetic.make_read(n_bases=n_bases, seed=seed)
    rw = rv.data_loader.prepare_windows(sig, stride=6, max_raw_len=T_R, max_event_len=T_E)
    raw_sc = rw.raw_sc.copy()
    raw_sc[ZERO_AT] = 0.0
    assert 400 < raw_sc.shape[0] < 900 and rw.events_sc.shape[0] > 30 and np.count_nonzero(raw_sc == 0.0) == 1
    return raw_sc, rw.events_sc.copy()


def _rows(N, E, mode="joint"):
    """The 19 hand-made rows (raw_start, raw_len, event_start, event_len); a mode that uses one segment only has no empty chunk."""
    rows = [(0, T_R, 0, T_E),                     # from sample 0 / event 0, full length: holds the 0.0 sample
            (N - T_R, T_R, E - T_E, T_E),         # ends on the last sample and the last event, full length
            (N - 17, 17, E - 3, 3),               # ends there too, short
            (5, 0, 4, 5),                         # no raw samples, real events
            (11, 23, 9, 0),                       # the reverse
            (1, 39, 1, 7), (3, 37, 3, 5), (ZERO_AT, 1, 5, 1), (ZERO_AT - 1, 3, 7, 2)]      # odd starts; the 0.0 sample first / in the middle
    rows += [(2 + i, T_R - (i % 7), 2 + i // 2, T_E - (i % 3)) for i in range(B - len(rows))]      # heavy overlap
    w = np.array(rows, np.int32)
    assert w.shape == (B, 4)
    if mode == "raw":
        w[w[:, 1] == 0, 1] = 1
    if mode == "event":
        w[w[:, 3] == 0, 3] = 1
    return w


def _mk(rv, mode, attention="luong", max_batch=B, **kw):
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=2, attention_type=attention,
                       honor_attention_type=True, max_batch=max_batch, max_raw_len=kw.get("T_r", T_R), max_event_len=kw.get("T_e", T_E),
                       max_output_len=kw.get("L", L))
    bc.set_weights_flat(_emitting_flat(rv, bc.cfg))
    return bc


def _ref(rv, bc, mode, read, rows, W):
    """The chunk-tensor call on the expanded rows -> (tokens, scores, S), read-only."""
    raw, ev = rv.data_loader.expand_windows(read[0], read[1], rows, T_R, T_E, 0.0)
    t, s = bc.beam_search_prediction(_x(mode, raw, ev), W, L)
    t, s = t.numpy().copy(), s.numpy().copy()
    t.setflags(write=False); s.setflags(write=False)
    return t, s, int(t.shape[1])


def _win(bc, table, W, **kw):
    return bc.beam_search_windows(table, W, L, T_r=T_R, T_e=T_E, **kw)


def _expands(bc):
    return int(bc.get_tensor("read_stats")[4])


def _taps(bc):
    return bc.get_tensor("mask").view(np.int32).copy(), bc.get_tensor("enc_output").view(np.int32).copy()


@pytest.fixture(scope="module")
def world(rv):
    """The joint Luong handle, one read put on it, its table and the chunk-tensor results per beam width, computed once."""
    bc = _mk(rv, "joint")
    read = _make_read(rv, seed=5)
    rows = _rows(read[0].shape[0], read[1].shape[0])
    handle = bc.put_read(*read)
    ref = {W: _ref(rv, bc, "joint", read, rows, W) for W in (1, 5)}
    assert ref[5][2] > 2 and len({r.tobytes() for r in ref[5][0]}) > B // 4 and len({r.tobytes() for r in ref[5][1]}) > B // 2, \
        "the chunks decode to different calls, with different scores"
    yield {"bc": bc, "read": read, "rows": rows, "handle": handle, "table": handle.table(rows), "ref": ref}
    bc.close()


@pytest.mark.parametrize("attention", ["luong", "bahdanau"])
@pytest.mark.parametrize("mode", ["raw", "event", "joint"])
def test_window_call_equals_padded_call(rv, mode, attention):
    bc = _mk(rv, mode, attention)
    read = _make_read(rv, seed=5)
    rows = _rows(read[0].shape[0], read[1].shape[0], mode)
    h = bc.put_read(read[0] if mode != "event" else None, read[1] if mode != "raw" else None)
    table = h.table(rows)
    for W in (1, 5):
        want = _ref(rv, bc, mode, read, rows, W)
        forms, (mask, enc) = bc.get_tensor("kernel_forms").copy(), _taps(bc)
        e0 = _expands(bc)
        got = _win(bc, table, W)
        assert _same(got, want), (mode, attention, W)
        assert np.array_equal(bc.get_tensor("kernel_forms"), forms), (mode, attention, W)
        wmask, wenc = _taps(bc)
        assert np.array_equal(wmask, mask) and np.array_equal(wenc, enc), (mode, attention, W)
        assert _expands(bc) == e0, "the default path gathers the windows in the recurrence's own prologue"
        if mode != "event":
            m = wmask.view(np.float32).reshape(B, -1)
            assert m[0, ZERO_AT] == 0.0 and m[0, ZERO_AT - 1] == 1.0 and m[0, ZERO_AT + 1] == 1.0, "a real 0.0 sample is masked"
            assert m[1, :T_R].all() and not m[2, 17:T_R].any()
        dev = _win(bc, table, W, device_outputs=True)
        assert _same(dev, want), (mode, attention, W, "device outputs")
    h.drop()
    bc.close()


FORMS = [({"wide_recurrence": 1}, 0), ({"wide_recurrence": 2}, 0), ({"wide_recurrence": 0}, 1), ({"lane_projection": 0}, 1),
         ({"debug_taps": 1}, 1), ({"persistent_decode": 0}, 1), ({"profile": 1}, 1), ({"slab_graph": 1}, 0)]


@pytest.mark.parametrize("opts,expands", FORMS, ids=["-".join(f"{k}{v}" for k, v in o.items()) for o, _ in FORMS])
def test_every_form_equals_its_padded_call(rv, world, opts, expands):
    bc, read, rows, table = world["bc"], world["read"], world["rows"], world["table"]
    try:
        for k, v in opts.items():
            bc.set_option(k, v)
        for W in (5, 1):
            want = _ref(rv, bc, "joint", read, rows, W)
            graph = "slab_graph" in opts
            forms, taps = (None if graph else bc.get_tensor("kernel_forms").copy()), _taps(bc)
            bc.reset_profile()
            e0 = _expands(bc)
            got = _win(bc, table, W)
            assert _same(got, want), (opts, W)
            assert _expands(bc) - e0 == expands, (opts, W)
            assert all(np.array_equal(a, b) for a, b in zip(_taps(bc), taps)), (opts, W)
            if not graph:      # (the padded call replayed a slab graph; a window call never does, and lists its forms)
                assert np.array_equal(bc.get_tensor("kernel_forms"), forms), (opts, W)
            else:
                assert len(bc.get_tensor("kernel_forms")) > 0
            if "profile" in opts:
                assert bc.profile()["expand_windows"][1] == 1
    finally:
        for k in opts:
            bc.set_option(k, {"wide_recurrence": 1, "lane_projection": 1, "persistent_decode": 1}.get(k, 0))


def test_fused_calls_equal_padded_calls(rv, world):
    bc, read, rows, table = world["bc"], world["read"], world["rows"], world["table"]
    raw, ev = rv.data_loader.expand_windows(read[0], read[1], rows, T_R, T_E, 0.0)
    for W in (5, 1):
        want = bc.beam_search_call_arrays((raw, ev), W, L)
        got = bc.beam_search_windows_call_arrays(table, W, L, T_r=T_R, T_e=T_E)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
        assert want[2].max() > 2


def test_asynchronous_and_coalesced_window_slabs(rv, world):
    bc, read, rows, table, ref = world["bc"], world["read"], world["rows"], world["table"], world["ref"]
    W = 5
    tables = [table[2:7], table, table[10:13], np.ascontiguousarray(table[::-1])]
    sync = []
    for t in tables:
        r = _win(bc, t, W)
        sync.append((r[0].numpy().copy(), r[1].numpy().copy(), int(r[0].shape[1])))
    assert _same((sync[1][0], sync[1][1]), ref[W])
    assert all(_same(sync[i], _ref(rv, bc, "joint", read, t[:, 1:], W)) for i, t in enumerate(tables))
    bc.set_async_depth(4)
    try:
        # no coalescing: a context per slab
        bc.set_coalesce(0)
        tickets = [bc.submit_windows(t, W, L, T_r=T_R, T_e=T_E) for t in tables]
        for i in (2, 0, 3, 1):
            assert _same(bc.collect(tickets[i]), sync[i]), i
        for side_ev, inplace, expands in ((-1, 1, 0), (0, 1, 0), (1, 1, 0), (0, 0, 2), (1, 0, 2)):
            bc.set_option("group_side_ev", side_ev)
            bc.set_option("group_inplace", inplace)
            bc.set_coalesce(2)
            g0, s0, _, in_force = _stats(bc)
            e0 = _expands(bc)
            assert in_force == 2
            tickets = [bc.submit_windows(t, W, L, T_r=T_R, T_e=T_E) for t in tables]      # 5 + 19 and 3 + 19: workgroups straddle the members
            g1, s1, largest, _ = _stats(bc)
            assert (g1 - g0, s1 - s0) == (2, 4) and largest >= 2, "two groups of two"
            for i, t in enumerate(tickets):
                assert _same(bc.collect(t), sync[i]), (side_ev, inplace, i)
            assert _expands(bc) - e0 == expands, (side_ev, inplace)
        bc.set_option("group_side_ev", -1)
        bc.set_option("group_inplace", 1)
        # fused post-processing through a group
        want = [bc.beam_search_windows_call_arrays(t, W, L, T_r=T_R, T_e=T_E) for t in tables[:2]]
        tickets = [bc.submit_windows(t, W, L, calls=True, T_r=T_R, T_e=T_E) for t in tables[:2]]
        for t, w in zip(tickets, want):
            got = bc.collect_calls(t)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, w))
        # a chunk-tensor slab between two window slabs: neither kind waits in the other's group
        raw, ev = rv.data_loader.expand_windows(read[0], read[1], tables[0][:, 1:], T_R, T_E, 0.0)
        g0, s0, _, _ = _stats(bc)
        ta = bc.submit_windows(tables[1], W, L, T_r=T_R, T_e=T_E)
        tb = bc.submit_beam_search((raw, ev), W, L)
        g1 = _stats(bc)[0]
        tc = bc.submit_windows(tables[2], W, L, T_r=T_R, T_e=T_E)
        g2 = _stats(bc)[0]
        assert (g1 - g0, g2 - g1) == (1, 1), "each submit of the other kind launched the group that was filling"
        assert _same(bc.collect(tb), sync[0]) and _same(bc.collect(tc), sync[2]) and _same(bc.collect(ta), sync[1])
        g3, s3, _, _ = _stats(bc)
        assert (g3 - g0, s3 - s0) == (3, 3), "three groups of one"
    finally:
        bc.set_option("group_side_ev", -1)
        bc.set_option("group_inplace", 1)
        bc.set_coalesce(-1)
        bc.set_async_depth(2)


def test_two_reads_in_one_slab_and_the_reads_lifetime(rv, world):
    bc, read_a, rows = world["bc"], world["read"], world["rows"]
    read_b = _make_read(rv, seed=9)
    Nb, Eb = read_b[0].shape[0], read_b[1].shape[0]
    rows_b = _rows(Nb, Eb)
    a0 = bc.get_tensor("read_stats")
    hb = bc.put_read(*read_b)
    a1 = bc.get_tensor("read_stats")
    assert a1[0] - a0[0] == 2 and a1[1] - a0[1] == 1, "a new read: one device buffer per table"
    table = world["handle"].table(rows)
    table[1::2] = hb.table(rows_b)[1::2]
    ra, ea = rv.data_loader.expand_windows(read_a[0], read_a[1], rows, T_R, T_E, 0.0)
    rb, eb = rv.data_loader.expand_windows(read_b[0], read_b[1], rows_b, T_R, T_E, 0.0)
    ra[1::2], ea[1::2] = rb[1::2], eb[1::2]
    t, s = bc.beam_search_prediction((ra, ea), 5, L)
    want = (t.numpy().copy(), s.numpy().copy(), int(t.shape[1]))
    assert not _same(world["ref"][5], want), "the second read decodes differently"
    assert _same(_win(bc, table, 5), want)
    # a read with an uncollected ticket cannot be dropped
    ticket = bc.submit_windows(table, 5, L, T_r=T_R, T_e=T_E)
    with pytest.raises(rv._capi.RavventHipError, match="RV_ESTATE"):
        hb.drop()
    assert _same(bc.collect(ticket), want)
    hb.drop()
    with pytest.raises(rv._capi.RavventHipError, match=r"RV_EINVAL.*row 1.*unknown read_id"):
        _win(bc, table, 5)
    # a put no larger than the buffers dropped allocates nothing, and is a new read with the new data
    a2 = bc.get_tensor("read_stats")
    hc = bc.put_read(read_b[0][::-1].copy(), read_b[1][: Eb - 1])
    a3 = bc.get_tensor("read_stats")
    assert a3[0] == a2[0] and a3[2] - a2[2] == 1 and a3[3] == a2[3] and hc.read_id != table[1, 0]
    rows_c = _rows(Nb, Eb - 1)
    rc, ec = rv.data_loader.expand_windows(read_b[0][::-1].copy(), read_b[1][: Eb - 1], rows_c, T_R, T_E, 0.0)
    t, s = bc.beam_search_prediction((rc, ec), 5, L)
    assert _same(_win(bc, hc.table(rows_c), 5), (t.numpy(), s.numpy(), int(t.shape[1])))
    hc.drop()


def test_device_reads_are_used_in_place(rv, world):
    import torch
    bc, read, rows = world["bc"], world["read"], world["rows"]
    pool = torch.zeros(1 + read[0].size + read[1].size + 2, dtype=torch.float32, device="cuda")
    raw = pool[1:1 + read[0].size]
    ev = pool[2 + read[0].size:2 + read[0].size + read[1].size].view(-1, 5)
    raw.copy_(torch.from_numpy(read[0])); ev.copy_(torch.from_numpy(read[1]))
    a0 = bc.get_tensor("read_stats")
    h = bc.put_read(raw, ev)
    assert bc.get_tensor("read_stats")[0] == a0[0], "no copy, no allocation"
    assert _same(_win(bc, h.table(rows), 5), world["ref"][5])
    h.drop()


BAD = [("unknown read_id", lambda t, N, E: t.__setitem__((3, 0), 12345)),
       ("negative raw start", lambda t, N, E: t.__setitem__((3, 1), -1)),
       ("negative event start", lambda t, N, E: t.__setitem__((3, 3), -2)),
       ("ends beyond the read's", lambda t, N, E: t.__setitem__((3, 1), N - t[3, 2] + 1)),
       ("events", lambda t, N, E: t.__setitem__((3, 3), E - t[3, 4] + 1)),
       ("exceeds T_r", lambda t, N, E: (t.__setitem__((3, 1), 0), t.__setitem__((3, 2), T_R + 1)))]


def test_bad_rows_are_refused_before_anything_is_queued(rv, world):
    bc, read, table = world["bc"], world["read"], world["table"]
    N, E = read[0].shape[0], read[1].shape[0]
    bc.set_option("profile", 1)
    try:
        bc.reset_profile()
        for what, spoil in BAD:
            t = table.copy()
            t[3, 1:] = (2, 5, 2, 5)
            spoil(t, N, E)
            for call in (lambda: _win(bc, t, 5), lambda: bc.beam_search_windows_call_arrays(t, 5, L, T_r=T_R, T_e=T_E),
                         lambda: bc.submit_windows(t, 5, L, T_r=T_R, T_e=T_E)):
                with pytest.raises(rv._capi.RavventHipError, match=r"RV_EINVAL: window row 3.*" + what):
                    call()
        assert all(n == 0 for _, n in bc.profile().values()), "nothing was launched"
    finally:
        bc.set_option("profile", 0)
    assert _same(_win(bc, table, 5), world["ref"][5]), "the next valid call is right"


def test_all_padding_chunk_among_ordinary_ones(rv, world):
    bc, read, rows, handle = world["bc"], world["read"], world["rows"].copy(), world["handle"]
    pos = 9
    rows[pos] = (13, 0, 6, 0)
    raw, ev = rv.data_loader.expand_windows(read[0], read[1], rows, T_R, T_E, 0.0)
    assert not raw[pos].any() and not ev[pos].any()
    for W in (5, 1):
        t, s = bc.beam_search_prediction((raw, ev), W, L)
        t, s = t.numpy(), s.numpy()
        wt, ws = _win(bc, handle.table(rows), W)
        wt, ws = wt.numpy(), ws.numpy()
        keep = [b for b in range(B) if b != pos]
        assert wt.shape == t.shape == (B, L - 1), "the padding chunk never finishes: the slab runs every step"
        assert np.array_equal(wt[keep], t[keep]) and np.array_equal(ws[keep].view(np.int32), s[keep].view(np.int32))
        # the chunk itself, as tests/test_padding_chunk_gpu.py compares such chunks: tokens exact, NaN where the reference has NaN
        assert np.array_equal(wt[pos], t[pos]) and (wt[pos] == 0).all()
        assert np.array_equal(np.isnan(ws), np.isnan(s)) and np.isnan(ws[pos]).all()


def test_basecall_end_to_end(rv):
    dl = rv.data_loader
    bc = _mk(rv, "joint", max_batch=32, T_r=dl.MAX_RAW_LEN, T_e=dl.MAX_EVENT_LEN, L=40)
    sig, labels = rv.synthetic.make_read(n_bases=300, seed=3)
    sig_b, _ = rv.synthetic.make_read(n_bases=120, seed=4)
    res = bc.basecall(sig, chunk_size=16)
    rw = dl.prepare_windows(sig, stride=6)
    raw, ev = rw.expand()
    n = len(rw)
    assert res.chunks_num == n and n > 2 * 16 and n % 16, "several slabs, the last one partial"
    parts = [bc.beam_search_call_arrays((raw[a:a + 16], ev[a:a + 16]), 5, 40) for a in range(0, n, 16)]
    seq, probs = rv.merger.Merger().merge_arrays(*[np.concatenate([p[k] for p in parts]) for k in range(3)])
    assert len(seq) > 100 and res.seq == seq and res.probs.tobytes() == probs.tobytes()
    assert res.qualities.shape == (len(seq),) and res.to_fastq("r").count("\n") == 4
    many = bc.basecall_many([sig, sig_b, sig], chunk_size=16)
    single_b = bc.basecall(sig_b, chunk_size=16)
    assert [m.seq for m in many] == [seq, single_b.seq, seq] and len(single_b.seq) > 30
    assert many[0].probs.tobytes() == probs.tobytes() and many[1].probs.tobytes() == single_b.probs.tobytes()
    assert int(bc.get_tensor("read_stats")[1]) == 0, "every read was dropped"
    ev_w = rv.evaluator.PerformanceEvaluator(bc, windows=True).run_read(sig, labels, chunk_size=16)
    ev_p = rv.evaluator.PerformanceEvaluator(bc, windows=False).run_read(sig, labels, chunk_size=16)
    assert ev_w["merged_seq"] == ev_p["merged_seq"] and len(ev_w["merged_seq"]) > 30
    assert ev_w["chunks_num"] == ev_p["chunks_num"] and set(ev_w) == set(ev_p)
    assert [s for s, _ in ev_w["nuc_preds"]] == [s for s, _ in ev_p["nuc_preds"]]
    bc.close()
