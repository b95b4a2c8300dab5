"""Stitching a read by signal position on the GPU (csrc/stitch.hip): rv_stitch_calls on tables made on the host
against the numpy statement of the rule (tests/stitch_reference.py), every output compared as bytes (NaN matching NaN); the refusals,
each by name with the next call succeeding; and basecall_many(merge="position") end to end against the rule applied to what the
calls-with-positions window call returns for the same tables.  No tolerance anywhere: nothing is summed."""
import ctypes
import os
import re

import numpy as np
import pytest

import signal_prep_inputs as SP
import stitch_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_THREADS = int(re.search(r"constexpr int ST_THREADS = (\d+);", open(os.path.join(ROOT, "ravvent-basecaller_amd", "csrc", "stitch.h")).read()).group(1))
NONE = np.zeros(0, np.int64)
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def _basecaller(rv, mode, rnn="bilstm", max_batch=32, L=64):
    return rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=2, decoder_depth=1, rnn_type=rnn,
                         max_batch=max_batch, max_raw_len=200, max_event_len=30, max_output_len=L)


@pytest.fixture(scope="module")
def bcs(rv):
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = _basecaller(rv, mode)
        return made[mode]
    yield get
    for bc in made.values():
        bc.close()


def _events(rng, E):
    ln = rng.integers(1, 30, E).astype(np.int64)
    st = (np.concatenate([[0], np.cumsum(ln)[:-1]]) if E else np.zeros(0)).astype(np.int64)
    return st, ln


def _read(rng, n, stride, lengths=None, E=None):
    """One read's tables: random, with NaNs, equal masses, integer event positions and positions beyond every interval."""
    E = int(rng.integers(1, 40)) if E is None else E
    st, ln = _events(rng, E)
    a = np.sort(rng.integers(0, 400, n))
    win = np.stack([a, rng.integers(0, 200, n), rng.integers(0, max(E, 1), n), rng.integers(0, 30, n)], axis=1).astype(np.int32).reshape(n, 4)
    f = lambda lo, hi: rng.uniform(lo, hi, (n, stride)).astype(np.float32)
    raw_pos = f(-20, 220)
    event_pos = np.where(rng.random((n, stride)) < 0.3, np.floor(f(-2, 45)), f(-2, 45)).astype(np.float32)
    raw_mass, event_mass = f(0, 1), f(0, 1)
    tie = rng.random((n, stride)) < 0.2
    event_mass[tie] = raw_mass[tie]
    for arr in (raw_pos, event_pos, raw_mass, event_mass):
        arr[rng.random((n, stride)) < 0.05] = np.nan
    if lengths is None:
        lengths = rng.choice(np.array([0, 1, stride]), n)
    return dict(win=win, bases=rng.choice(LETTERS, (n, stride)), probs=f(0, 1), lengths=np.asarray(lengths, np.int32), raw_pos=raw_pos,
                raw_mass=raw_mass, event_pos=event_pos, event_mass=event_mass, st=st, ln=ln)


class _Moves:
    def __init__(self, d):
        self.raw_pos, self.raw_mass, self.event_pos, self.event_mass = d["raw_pos"], d["raw_mass"], d["event_pos"], d["event_mass"]


def _put(bc, reads):
    """Reads on the device that the tables can name: empty scaled tables of the right lengths, and the events."""
    hs = []
    for d in reads:
        E = len(d["st"])
        hs.append(bc.put_read(np.zeros(8, np.float32), np.zeros((E, 5), np.float32), event_starts=d["st"], event_lengths=d["ln"]))
    return hs


def _tables(reads, hs):
    cat = lambda k: np.concatenate([d[k] for d in reads])
    table = np.concatenate([h.table(d["win"]) for h, d in zip(hs, reads)]).astype(np.int32).reshape(-1, 5)
    rows = np.concatenate([[0], np.cumsum([len(d["lengths"]) for d in reads])]).astype(np.int32)
    t = dict(table=table, rows=rows, **{k: cat(k) for k in ("bases", "probs", "lengths", "raw_pos", "raw_mass", "event_pos", "event_mass")})
    return t


def _check(bc, mode, reads, tag):
    """rv_stitch_calls on the reads' tables against the reference -> the device result."""
    hs = _put(bc, reads)
    try:
        t = _tables(reads, hs)
        got = bc.stitch_calls(t["bases"], t["probs"], t["lengths"], _Moves(t), t["table"], t["rows"])
        want, offs = R.stitch(mode, t["table"], t["rows"], t["bases"], t["probs"], t["lengths"], t["raw_pos"], t["raw_mass"], t["event_pos"],
                              t["event_mass"], [(d["st"], d["ln"]) for d in reads])
        assert got.read_offsets.tobytes() == offs.tobytes(), (tag, "read_offsets", got.read_offsets.tolist(), offs.tolist())
        for k, g, w in zip(R.FIELDS, got[:7], want):
            assert R.same_bits(g, w), (tag, k, g[:8].tolist(), w[:8].tolist())
        return got
    finally:
        for h in hs:
            h.drop()


@pytest.mark.parametrize("mode", ["joint", "raw", "event"])
def test_against_reference(bcs, mode):
    """Row strides 1, 2 and 63; lengths 0, 1 and full; reads of 0, 1, 2 and 17 chunks; three reads with an empty one in the middle."""
    bc = bcs(mode)
    rng = np.random.default_rng({"joint": 11, "raw": 12, "event": 13}[mode])
    kept = 0
    for stride in (1, 2, 63):
        for counts in ([0], [1], [2], [17], [0, 1, 2, 17], [3, 0, 4]):
            got = _check(bc, mode, [_read(rng, n, stride) for n in counts], (mode, stride, counts))
            kept += len(got.bases)
        full = _check(bc, mode, [_read(rng, 17, stride, lengths=np.full(17, stride))], (mode, stride, "full"))
        kept += len(full.bases)
    assert kept > 200, ("vacuous", mode, kept)


def _plain(win, raw_pos, lengths=None, **kw):
    """A read whose positions are raw_start + raw_pos (raw mass 1, event mass 0 unless given)."""
    win = np.asarray(win, np.int32).reshape(-1, 4)
    raw_pos = np.asarray(raw_pos, np.float32)
    n, stride = raw_pos.shape
    d = dict(win=win, bases=np.tile(LETTERS, n * stride)[:n * stride].reshape(n, stride).copy(), probs=np.full((n, stride), 0.25, np.float32),
             lengths=np.full(n, stride, np.int32) if lengths is None else np.asarray(lengths, np.int32), raw_pos=raw_pos,
             raw_mass=np.ones((n, stride), np.float32), event_pos=np.full((n, stride), -1, np.float32),
             event_mass=np.zeros((n, stride), np.float32), st=np.array([0, 10, 30], np.int64), ln=np.array([10, 20, 7], np.int64))
    d.update({k: np.asarray(v, np.float32) for k, v in kw.items()})
    return d


def test_edges_of_the_rule(bcs):
    bc = bcs("joint")
    below = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))
    # centres 100 and 200: the cut is 150.  A position exactly on it goes to the later chunk; its float32 neighbour below to the earlier
    w2 = [[0, 200, 0, 3], [100, 200, 0, 3]]
    got = _check(bc, "joint", [_plain(w2, [[10, 150, below(150)], [below(50), 50, 60]], lengths=[3, 3])], "cut")
    assert got.source_chunk.tolist() == [0, 0, 0, 1, 1] and got.source_index.tolist() == [0, 1, 2, 1, 2]      # (150 in chunk 0: inside the hull)
    got = _check(bc, "joint", [_plain(w2, [[10, below(150), 150], [50, below(50), 60]], lengths=[3, 3])], "cut2")
    assert got.source_chunk.tolist() == [0, 0, 1, 1, 1] and got.positions[1] < 150 and got.positions[2] == 150
    # equal centres 50, 70, 70, 70: the cuts are 60, 70, 70, and the interval of chunk 2 is [70, 70): empty, whatever it called
    w4 = [[0, 100, 0, 3], [20, 100, 0, 3], [20, 100, 0, 3], [20, 100, 0, 3]]
    got = _check(bc, "joint", [_plain(w4, [[10, 20, 59.9]] + [[39.9, 40, 50]] * 3)], "equal centres")
    assert got.source_chunk.tolist() == [0, 0, 0, 1, 3] and got.positions.tolist()[3:] == [60.0, 70.0]
    # a chunk with no inside base, an all-NaN chunk, and non-monotone positions: the hull keeps the base between two inside ones
    nan = np.nan
    w3 = [[0, 200, 0, 3], [100, 200, 0, 3], [200, 200, 0, 3]]
    got = _check(bc, "joint", [_plain(w3, [[500, 600, 700, 800], [nan, nan, nan, nan], [80, 900, -500, 90]])], "hull")
    assert got.source_chunk.tolist() == [2, 2, 2, 2] and got.positions.tolist() == [280.0, 1100.0, -300.0, 290.0]
    got = _check(bc, "joint", [_plain(w3, [[500, 100, 700, 800], [60, nan, 5000, 70], [nan, 90, nan, nan]])], "nan inside the hull")
    assert got.source_chunk.tolist() == [0, 1, 1, 1, 1, 2] and np.isnan(got.positions[2])
    # joint rows at raw_mass == event_mass take the raw estimate; a mass below takes the event estimate (events: centres 5, 20, 33.5)
    d = _plain([[0, 200, 0, 3], [100, 200, 1, 2]], [[10, 20, 30], [60, 50, 60]], event_pos=[[0, 1, 1.5], [0, 0.5, 7]],
               raw_mass=[[0.5, 0.5, 0.25], [0.5, 0.25, 0.25]], event_mass=[[0.5, 0.25, 0.5], [0.5, 0.5, 0.5]])
    got = _check(bc, "joint", [d], "ties")
    assert got.positions.tolist() == [10.0, 20.0, 20.0 + 0.5 * 13.5, 160.0], got.positions.tolist()


def test_event_positions(bcs):
    """An event position that is an exact integer, one at E - 1, and one beyond it; a read without events gives NaN everywhere."""
    bc = bcs("event")
    st, ln = np.array([0, 10, 30, 37], np.int64), np.array([10, 20, 7, 4], np.int64)           # centres 5, 20, 33.5, 39
    d = _plain([[0, 20, 0, 3], [20, 20, 1, 3]], [[0, 0, 0, 0, 0]] * 2, event_pos=[[0, 1, 2.5, 3, 9], [0.25, 1, 2, 2.5, -4]],
               event_mass=np.ones((2, 5)), raw_mass=np.zeros((2, 5)))
    d["st"], d["ln"] = st, ln
    got = _check(bc, "event", [d], "event")
    # chunk 0 owns (-inf, 20): events 0, 1 (centre 20 is the cut: not inside), the hull ends at index 0; chunk 1 owns [20, inf)
    assert got.source_chunk.tolist() == [0, 1, 1, 1, 1] and got.positions.tolist() == [5.0, 20.0 + 0.25 * 13.5, 33.5, 39.0, 39.0]
    e = dict(d, st=NONE, ln=NONE)
    got = _check(bc, "event", [e], "no events")
    assert len(got.bases) == 0 and got.read_offsets.tolist() == [0, 0]


def test_scan_tile_edges(bcs):
    """Chunk counts on both sides of every edge of the scan: its tile of ST_THREADS chunks (one workgroup), two tiles, and
    ST_THREADS tiles, beyond which a thread of the carry pass takes more than one tile -- the multi-workgroup path from the second
    count on.  Stride 1, raw mode, five reads with an empty one among them."""
    bc = bcs("raw")
    T = ST_THREADS
    rng = np.random.default_rng(21)
    for n in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, T * T - 1, T * T, T * T + 1):
        cuts = np.sort(rng.integers(0, n + 1, 3))
        counts = np.diff(np.concatenate([[0], cuts[:2], cuts[1:2], cuts[2:], [n]]))                 # (the third read is empty)
        reads = []
        for m in counts:
            a = np.arange(m, dtype=np.int64) * 7
            win = np.stack([a, np.full(m, 20), np.zeros(m, np.int64), np.zeros(m, np.int64)], axis=1)
            # positions around the chunk's own interval [a + 6.5, a + 13.5): about half of them inside
            reads.append(_plain(win, rng.uniform(3, 17, (m, 1)), lengths=rng.choice(np.array([0, 1, 1, 1]), m)))
        got = _check(bc, "raw", reads, ("scan", n))
        assert 0 < len(got.bases) < n, (n, len(got.bases))


def test_profile_scopes(bcs):
    """Under option "profile" a stitch leaves one entry per stage; a stitch that keeps nothing runs no scatter."""
    bc = bcs("raw")
    d = _plain([[0, 200, 0, 0], [100, 200, 0, 0]], [[10, 150], [20, 50]])
    bc.set_option("profile", 1)
    try:
        bc.reset_profile()
        _check(bc, "raw", [d], "profile")
        prof = bc.profile()
        assert {k: prof[k][1] for k in ("stitch_keep", "stitch_scan", "stitch_scatter")} == dict(stitch_keep=1, stitch_scan=1, stitch_scatter=1), prof
        assert all(prof[k][0] > 0 for k in ("stitch_keep", "stitch_scan", "stitch_scatter")), prof
        _check(bc, "raw", [dict(d, lengths=np.zeros(2, np.int32))], "profile, nothing kept")
        prof = bc.profile()
        assert (prof["stitch_keep"][1], prof["stitch_scan"][1], prof["stitch_scatter"][1]) == (2, 2, 1), prof
    finally:
        bc.set_option("profile", 0)
        bc.reset_profile()


def _raw_call(bc, rv, t, cap, n_reads):
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    cin = rv._capi.CRvStitchIn(p(t["bases"]), p(t["probs"]), p(t["lengths"]), p(t["raw_pos"]), p(t["raw_mass"]), p(t["event_pos"]),
                               p(t["event_mass"]), p(t["table"]), len(t["lengths"]), t["bases"].shape[1])
    arrs, cout = bc._stitch_out(cap, n_reads)
    for a in arrs[:7]:
        a.view(np.uint8)[:] = 0xA5
    rc = bc._lib.rv_stitch_calls(bc._h, ctypes.byref(cin), n_reads, p(t["rows"]), ctypes.byref(cout))
    return rc, arrs, (bc._lib.rv_last_error(bc._h) or b"").decode()


def test_capacity_and_refusals(rv, bcs):
    bc = bcs("joint")
    err = rv._capi.RavventHipError
    rng = np.random.default_rng(31)
    reads = [_read(rng, 6, 5, lengths=np.full(6, 5), E=12), _read(rng, 5, 5, lengths=np.full(5, 5), E=9)]
    hs = _put(bc, reads)
    try:
        t = _tables(reads, hs)
        mv = _Moves(t)
        ok = bc.stitch_calls(t["bases"], t["probs"], t["lengths"], mv, t["table"], t["rows"])
        total = len(ok.bases)
        assert total > 2
        # a capacity one element short: RV_EINVAL with the size needed, the offsets written, the outputs untouched
        rc, arrs, msg = _raw_call(bc, rv, t, total - 1, 2)
        assert rc == -1 and f"hold {total} bases" in msg and f"room for {total - 1}" in msg, (rc, msg)
        assert arrs[7].tobytes() == ok.read_offsets.tobytes() and all((a.view(np.uint8) == 0xA5).all() for a in arrs[:7])
        rc, arrs, msg = _raw_call(bc, rv, t, total, 2)
        assert rc == 0 and all(R.same_bits(a[:total], b) for a, b in zip(arrs[:7], ok[:7]))
        # an unknown read, and a row in another read's rows: refused by name, and the next call is the first one again
        bad = t["table"].copy()
        bad[3, 0] = 12345678
        with pytest.raises(err, match=r"RV_EINVAL: rv_stitch_calls: row 3: unknown read_id 12345678"):
            bc.stitch_calls(t["bases"], t["probs"], t["lengths"], mv, bad, t["rows"])
        bad = t["table"].copy()
        bad[4, 0] = t["table"][7, 0]
        with pytest.raises(err, match=r"RV_EINVAL: rv_stitch_calls: row 4 names read \d+, but lies in the rows \[0,6\) of read"):
            bc.stitch_calls(t["bases"], t["probs"], t["lengths"], mv, bad, t["rows"])
        with pytest.raises(err, match=r"RV_EINVAL: rv_stitch_calls: read_rows\[2\] = 12 lies outside the table's 11 rows"):
            bc.stitch_calls(t["bases"], t["probs"], t["lengths"], mv, t["table"], np.array([0, 6, 12], np.int32))
        again = bc.stitch_calls(t["bases"], t["probs"], t["lengths"], mv, t["table"], t["rows"])
        assert all(R.same_bits(a, b) for a, b in zip(again, ok))
        # a read without an event table on the device: RV_ESTATE by name in joint mode; rv_read_put_events then serves it
        h = bc.put_read(np.zeros(8, np.float32), np.zeros((len(reads[0]["st"]), 5), np.float32))
        try:
            t2 = _tables(reads[:1], [h])
            with pytest.raises(err, match=r"RV_ESTATE: rv_stitch_calls: read \d+ has no event table on the device.*rv_read_put_events"):
                bc.stitch_calls(t2["bases"], t2["probs"], t2["lengths"], _Moves(t2), t2["table"], t2["rows"])
            with pytest.raises(err, match=r"RV_EINVAL: rv_read_put_events: 2 events for read \d+, whose event table holds"):
                bc._check(bc._lib.rv_read_put_events(bc._h, h.read_id, ctypes.c_void_p(reads[0]["st"].ctypes.data),
                                                     ctypes.c_void_p(reads[0]["ln"].ctypes.data), 2), "rv_read_put_events")
            bc._check(bc._lib.rv_read_put_events(bc._h, h.read_id, ctypes.c_void_p(reads[0]["st"].ctypes.data),
                                                 ctypes.c_void_p(reads[0]["ln"].ctypes.data), len(reads[0]["st"])), "rv_read_put_events")
            one = bc.stitch_calls(t2["bases"], t2["probs"], t2["lengths"], _Moves(t2), t2["table"], t2["rows"])
            n0 = int(ok.read_offsets[1])
            assert all(R.same_bits(a, b[:n0]) for a, b in zip(one[:7], ok[:7]))
        finally:
            h.drop()
    finally:
        for h in hs:
            h.drop()
    # a read made from its signal holds its events already
    hsig = bc.put_signal(SP.step_signal(400))
    try:
        with pytest.raises(err, match=r"RV_ESTATE: read \d+ was made by rv_read_put_signals"):
            bc._check(bc._lib.rv_read_put_events(bc._h, hsig.read_id, None, None, 0), "rv_read_put_events")
    finally:
        hsig.drop()
    # raw mode needs no event table
    rawbc = bcs("raw")
    h = rawbc.put_read(np.zeros(8, np.float32), None)
    try:
        d = _plain([[0, 200, 0, 0], [100, 200, 0, 0]], [[10, 150], [20, 50]])
        t3 = _tables([d], [h])
        got = rawbc.stitch_calls(t3["bases"], t3["probs"], t3["lengths"], _Moves(t3), t3["table"], t3["rows"])
        assert got.positions.tolist() == [10.0, 150.0]
    finally:
        h.drop()


def _device_path_refusals(rv, bc, sig, Lr):
    """Tickets into a stitch buffer that are uncollected at rv_stitch_run / rv_stitch_close, rows outside it, the wrong collect."""
    err = rv._capi.RavventHipError
    lib, hd = bc._lib, bc._h
    h = bc.put_signal(sig, stride=6, max_raw_len=200, max_event_len=30)
    sb = ctypes.c_void_p()
    try:
        tab = h.table(h.windows)[:4]
        bc._check(lib.rv_stitch_open(hd, 4, Lr, ctypes.byref(sb)), "rv_stitch_open")
        lut = bc._call_lut()
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        t, S = ctypes.c_int32(-1), ctypes.c_int32(0)
        sub = lambda B, row0, L=Lr: lib.rv_beam_search_submit_windows_stitch(hd, p(tab), B, 200, 30, 5, L, p(lut), sb, row0, ctypes.byref(t))
        with pytest.raises(err, match=r"RV_EINVAL: rows \[1,5\) lie outside the stitch buffer's 4 rows"):
            bc._check(sub(4, 1), "submit")
        with pytest.raises(err, match=rf"RV_EINVAL: max_output_len={Lr - 1}, but the stitch buffer was opened for {Lr}"):
            bc._check(sub(4, 0, Lr - 1), "submit")
        bc._check(sub(4, 0), "submit")
        rows = np.array([0, 4], np.int32)
        arrs, cout = bc._stitch_out(4 * (Lr - 1), 1)
        with pytest.raises(err, match=r"RV_ESTATE: rv_stitch_run: 1 uncollected ticket"):
            bc._check(lib.rv_stitch_run(hd, sb, 1, p(rows), ctypes.byref(cout)), "rv_stitch_run")
        with pytest.raises(err, match=r"RV_ESTATE: rv_stitch_close: 1 uncollected ticket"):
            bc._check(lib.rv_stitch_close(hd, sb), "rv_stitch_close")
        with pytest.raises(err, match=r"RV_EINVAL: this call's results went to a stitch buffer: collect it with rv_beam_search_collect_stitch"):
            bc.collect_calls_moves({"ticket": t.value, "B": 4, "steps": Lr - 1})
        with pytest.raises(err, match=r"RV_ESTATE: read \d+ is used by 1 uncollected ticket"):
            h.drop()
        bc._check(lib.rv_beam_search_collect_stitch(hd, t.value, ctypes.byref(S)), "collect")
        assert S.value == Lr - 1
        with pytest.raises(err, match=r"RV_EINVAL: rv_stitch_run: read_rows\[1\] = 5 lies outside the table's 4 rows"):
            bc._check(lib.rv_stitch_run(hd, sb, 1, p(np.array([0, 5], np.int32)), ctypes.byref(cout)), "rv_stitch_run")
        bc._check(lib.rv_stitch_run(hd, sb, 1, p(rows), ctypes.byref(cout)), "rv_stitch_run")
        # the other way round: a ticket of the calls-with-positions submit is not the stitch collect's
        call = bc.submit_windows(tab, 5, Lr, calls=True, T_r=200, T_e=30, moves=True)
        with pytest.raises(err, match=r"RV_EINVAL: rv_beam_search_collect_stitch takes the tickets of rv_beam_search_submit_windows_stitch"):
            bc._check(lib.rv_beam_search_collect_stitch(hd, call["ticket"], ctypes.byref(S)), "collect")
        bc.collect_calls_moves(call)
    finally:
        if sb:
            lib.rv_stitch_close(hd, sb)
        h.drop()


def _same_result(a, b):
    return (a.seq == b.seq and a.chunks_num == b.chunks_num and a.probs.tobytes() == b.probs.tobytes() and
            a.qualities.tobytes() == b.qualities.tobytes())


@pytest.mark.parametrize("rnn", ["bilstm", "bigru"])
def test_end_to_end(rv, rnn):
    """basecall_many(merge="position") equals the rule applied to what beam_search_windows_calls_moves returns for the same tables,
    field for field as bytes: host and device preparation, slabs of 7 chunks (which span reads) and one slab of all; the alignment
    merge returns the same bytes before and after.  base_calling_weights: every call is full length."""
    Lr, W, mode = 24, 5, "joint"
    sigs = [SP.step_signal(1500), SP.step_signal(40), np.asarray(SP.synthetic_signal(rv, 120, 11)).astype(np.int16)]
    bc = _basecaller(rv, mode, rnn=rnn, max_batch=32, L=Lr)
    try:
        bc.set_weights_flat(rv.weights.base_calling_weights(bc.cfg))
        before = bc.basecall_many(sigs, max_output_len=Lr, chunk_size=7)
        kept = chunks = 0
        for dev in (False, True):
            # the tables and events of this preparation, and the chunk-level calls with positions on them
            if dev:
                hs = bc.put_signals(sigs, stride=6, max_raw_len=200, max_event_len=30)
                wins = [h.windows for h in hs]
                evs = [(h.fetch("start"), h.fetch("length")) if h.n_event else (NONE, NONE) for h in hs]
            else:
                hs, wins, evs = [], [], []
                for sig in sigs:
                    rw = rv.data_loader.prepare_windows(sig, stride=6, max_raw_len=200, max_event_len=30)
                    st, ln, _, _ = rv.event_detection.EventDetector(window_length1=rv.data_loader.ED_WINDOW_LENGTH_1,
                                                                     window_length2=rv.data_loader.ED_WINDOW_LENGTH_2).run_arrays(np.asarray(sig))
                    hs.append(bc.put_read(rw.raw_sc, rw.events_sc))
                    wins.append(rw.windows)
                    evs.append((np.asarray(st, np.int64), np.asarray(ln, np.int64)))
            try:
                table = np.concatenate([h.table(w) for h, w in zip(hs, wins)])
                rows = np.concatenate([[0], np.cumsum([len(w) for w in wins])]).astype(np.int32)
                assert len(table) <= 32 and len(wins[1]) == 0 and min(len(wins[0]), len(wins[2])) >= 8
                bases, probs, lens, mv = bc.beam_search_windows_calls_moves(table, W, Lr, T_r=200, T_e=30)
            finally:
                for h in hs:
                    h.drop()
            assert (lens == Lr - 1).all(), "base_calling_weights: every call is full length"
            want, offs = R.stitch(mode, table, rows, bases, probs, lens, mv.raw_pos, mv.raw_mass, mv.event_pos, mv.event_mass, evs)
            for cs in (7, 1024):
                res = bc.basecall_many(sigs, max_output_len=Lr, chunk_size=cs, device_prep=dev, merge="position")
                assert len(res) == 3
                for i, r in enumerate(res):
                    a, b = int(offs[i]), int(offs[i + 1])
                    tag = (rnn, dev, cs, i)
                    assert r.seq.encode() == want[0][a:b].tobytes() and r.chunks_num == len(wins[i]), (tag, "seq")
                    for k, g, w in zip(R.FIELDS[1:], (r.probs, r.positions, r.raw_mass, r.event_mass, r.source_chunk, r.source_index), want[1:]):
                        assert R.same_bits(g, w[a:b]), (tag, k)
                    assert r.qualities.tobytes() == rv.basecaller.phred_qualities(want[1][a:b]).tobytes(), tag
                assert res[1].seq == "" and len(res[1].positions) == 0
            kept += int(offs[-1])
            chunks += len(set(want[5][:int(offs[1])].tolist()))
            print(f"{rnn} device_prep={dev}: {int(offs[-1])} bases kept of {int(lens.sum())} called, read 0 from {len(set(want[5][:int(offs[1])].tolist()))} chunks")
        assert kept > 0, "vacuous: no base of any read lies on its own chunk's stretch of signal"
        after = bc.basecall_many(sigs, max_output_len=Lr, chunk_size=7)
        assert all(_same_result(a, b) for a, b in zip(before, after)), "merge='align' changed across a stitched call"
        moved = bc.basecall_many(sigs, max_output_len=Lr, chunk_size=7, moves=True)
        assert all(_same_result(a, b) for a, b in zip(before, moved))
        if rnn == "bilstm":
            _device_path_refusals(rv, bc, sigs[0], Lr)
            again = bc.basecall_many(sigs, max_output_len=Lr, chunk_size=7)
            assert all(_same_result(a, b) for a, b in zip(before, again))
        with pytest.raises(ValueError, match="merge 'nearest'"):
            bc.basecall_many(sigs, merge="nearest")
    finally:
        bc.close()
