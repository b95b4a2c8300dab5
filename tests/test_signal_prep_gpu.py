"""Reads prepared on the device from their int16 samples (rv_read_put_signals, csrc/signal_prep.hip), held to the
host path of the same library:

  events        bit-equal to EventDetector.run_arrays (start, length; mean and stdv as fp64 bit patterns), and on the event fixtures
                start / length also equal to the reference's own output
  window table  equal to data_loader.prepare_windows(...).windows
  scaled tables equal or adjacent in float32, a zero exactly zero, at most 1 element in 10,000 different (signal_prep_inputs)
  decode        a window call on such a read returns the bytes of the padded call on expand_windows of the tables fetched from it
  batches       byte for byte their reads put one by one

Signals and their proofs: tests/signal_prep_inputs.py, tests/test_signal_prep.py."""
import os

import numpy as np
import pytest

import signal_prep_inputs as spi
from test_coalesce_gpu import _same
from test_parity_gpu import _emitting_flat

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T_R, T_E, L = 40, 8, 8
CHUNKER = dict(stride=6, max_raw_len=200, max_event_len=30)       # the chunker's own parameters, whatever the handle was sized for
TABLES = ("windows", "raw_sc", "events_sc", "start", "length", "mean", "stdv")


def _mk(rv, mode="joint", max_batch=16):
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=2, attention_type="luong",
                       honor_attention_type=True, max_batch=max_batch, max_raw_len=T_R, max_event_len=T_E, max_output_len=L)
    bc.set_weights_flat(_emitting_flat(rv, bc.cfg))
    return bc


@pytest.fixture(scope="module")
def bc(rv):
    b = _mk(rv)
    yield b
    b.close()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _check_events(rv, h, sig, w1=6, w2=9):
    """The read's four event arrays against the host detector, bit for bit -> the host's arrays."""
    st, ln, mu, sd = rv.event_detection.EventDetector(window_length1=w1, window_length2=w2).run_arrays(np.asarray(sig))
    assert h.n_event == len(st), (len(sig), h.n_event, len(st))
    assert np.array_equal(h.fetch("start"), st) and np.array_equal(h.fetch("length"), ln), len(sig)
    assert np.array_equal(_bits(h.fetch("mean")), _bits(mu)), ("mean", len(sig))
    assert np.array_equal(_bits(h.fetch("stdv")), _bits(sd)), ("stdv", len(sig))
    return st, ln, mu, sd


def _check_read(rv, h, sig, **kw):
    """Everything of a read put at the chunker's own detector (6 / 9) against prepare_windows with the same parameters."""
    sig = np.asarray(sig)
    if sig.size == 0:
        assert h.n_raw == 0 and h.n_event == 0 and h.windows.shape == (0, 4)
        return
    _check_events(rv, h, sig)
    rw = rv.data_loader.prepare_windows(sig, **kw)
    assert h.windows.dtype == np.int32 and h.windows.shape == rw.windows.shape and np.array_equal(h.windows, rw.windows), (len(sig), kw)
    for name, want in (("raw_sc", rw.raw_sc), ("events_sc", rw.events_sc)):
        bad = spi.scaled_table_mismatch(h.fetch(name), want)
        assert bad is None, (name, len(sig), kw, bad)


@pytest.mark.parametrize("name", ["events_w6_9", "events_w3_6", "events_w6_6"])
def test_event_fixtures_at_their_own_windows(rv, bc, name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    w1, w2 = int(g["w"][0]), int(g["w"][1])
    h = bc.put_signal(g["signal"], detector=rv.event_detection.EventDetector(window_length1=w1, window_length2=w2))
    _check_events(rv, h, g["signal"], w1, w2)
    assert np.array_equal(h.fetch("start"), g["start"]) and np.array_equal(h.fetch("length"), g["length"]), "the reference's own events"
    assert h.n_event > 100
    h.drop()


@pytest.mark.parametrize("kind", ["step", "plateau"])
def test_every_start_up_length_and_both_sides_of_the_tiles(rv, bc, kind):
    make = {"step": spi.step_signal, "plateau": spi.plateau_signal}[kind]
    sigs = [make(n) for n in spi.LENGTHS]
    hs = bc.put_signals(sigs, **CHUNKER)
    assert [h.n_raw for h in hs] == spi.LENGTHS
    for h, sig in zip(hs, sigs):
        _check_read(rv, h, sig, **CHUNKER)
    assert hs[0].n_event == 0 and hs[70].n_event >= 4 and hs[-1].n_event > 4000 and len(hs[-1].windows) > 600
    for h in hs:
        h.drop()


def test_largest_read_and_the_refusal_beyond_it(rv, bc):
    n = spi.MAX_SAMPLES
    sig = spi.plateau_signal(n, period=64)
    h = bc.put_signal(sig, **CHUNKER)
    st, ln, _, _ = _check_events(rv, h, sig)
    assert h.n_event > 60000
    # (the host's loop over the chunks is quadratic in the events; its closed form is held to it in tests/test_signal_prep.py)
    rg = rv.data_loader.fitting_event_ranges_closed_form(ln, 6, 200)
    want = np.column_stack((st[rg[:, 0]], np.minimum(np.maximum(st[rg[:, 1] - 1] - st[rg[:, 0]], 0), 200),
                            rg[:, 0], np.minimum(rg[:, 1] - rg[:, 0], 30))).astype(np.int32)
    assert np.array_equal(h.windows, want)
    x = sig.astype(np.float64)
    bad = spi.scaled_table_mismatch(h.fetch("raw_sc"), ((x - x.mean()) / x.std()).astype(np.float32))
    assert bad is None, bad
    h.drop()
    alive = int(bc.get_tensor("read_stats")[1])
    with pytest.raises(rv._capi.RavventHipError, match="RV_EUNSUPPORTED.*2\\^22"):
        bc.put_signal(np.zeros(n + 1, np.int16))
    assert int(bc.get_tensor("read_stats")[1]) == alive, "a refused put makes no read"
    h = bc.put_signal(spi.step_signal(300), **CHUNKER)       # the handle works on
    _check_read(rv, h, spi.step_signal(300), **CHUNKER)
    h.drop()


def test_refusals_by_name_make_no_read(rv, bc):
    alive = int(bc.get_tensor("read_stats")[1])
    det = rv.event_detection.EventDetector
    for kw, code in ((dict(detector=det(window_length1=9, window_length2=6)), "RV_EINVAL"), (dict(detector=det(window_length1=0, window_length2=6)), "RV_EINVAL"),
                     (dict(stride=0), "RV_EINVAL"), (dict(max_raw_len=0), "RV_EINVAL")):
        with pytest.raises(rv._capi.RavventHipError, match=code):
            bc.put_signal(spi.step_signal(100), **kw)
    with pytest.raises(rv._capi.RavventHipError, match="RV_ESTATE"):
        bc.put_signals([np.zeros(0, np.int16)] * 1025)
    assert int(bc.get_tensor("read_stats")[1]) == alive
    with pytest.raises(ValueError, match="host path"):
        bc.put_signal(np.array([1.5, 2.0]))


def test_flat_and_one_event_reads(rv, bc):
    h = bc.put_signal(spi.flat_signal(), **CHUNKER)
    assert h.fetch("start").tolist() == [0] and h.fetch("length").tolist() == [2]
    assert not h.fetch("raw_sc").any(), "a zero deviation scales by 1"
    assert h.windows.shape == (0, 4)
    _check_read(rv, h, spi.flat_signal(), **CHUNKER)
    h.drop()
    h = bc.put_signal(spi.one_event_signal(), **CHUNKER)
    assert h.n_event == 1 and h.fetch("events_sc").shape == (1, 5) and not h.fetch("events_sc").any()
    _check_read(rv, h, spi.one_event_signal(), **CHUNKER)
    h.drop()


@pytest.fixture(scope="module")
def window_signals(rv):
    out = {n: np.load(os.path.join(GOLD, n + ".npz"), allow_pickle=True)["signal"] for n in ("chunks_a", "chunks_b", "chunks_c")}
    out["make_read"] = spi.synthetic_signal(rv, 1500, 11)
    return out


@pytest.mark.parametrize("kw", [dict(stride=6, max_raw_len=200, max_event_len=30), dict(stride=4), dict(stride=1),
                                dict(stride=6, max_raw_len=20), dict(stride=6, max_event_len=3)],
                         ids=["6-200-30", "stride4", "stride1", "raw20", "event3"])
@pytest.mark.parametrize("name", ["chunks_a", "chunks_b", "chunks_c", "make_read"])
def test_window_tables(rv, bc, window_signals, name, kw):
    sig = window_signals[name]
    kw = dict(CHUNKER, **kw)
    h = bc.put_signal(sig, **kw)
    _check_read(rv, h, sig, **kw)
    assert len(h.windows) > 20
    h.drop()


def test_batch_equals_its_reads_one_by_one(rv, bc):
    sigs = [spi.synthetic_signal(rv, 66, 5), np.zeros(0, np.int16), spi.flat_signal(), spi.plateau_signal(2500)]
    kw = dict(stride=4, max_raw_len=T_R, max_event_len=T_E)
    batch = bc.put_signals(sigs, **kw)
    assert batch[1].n_raw == 0 and batch[1].n_event == 0 and len(batch[1].windows) == 0, "the empty read"
    assert batch[2].n_event == 1 and len(batch[2].windows) == 0, "a read without windows"
    assert len(batch[0].windows) > 5 and len(batch[3].windows) > 5
    for hb, sig in zip(batch, sigs):
        one = bc.put_signal(sig, **kw)
        assert (hb.n_raw, hb.n_event) == (one.n_raw, one.n_event)
        assert hb.windows.tobytes() == one.windows.tobytes()
        for t in TABLES[1:]:
            assert hb.fetch(t).tobytes() == one.fetch(t).tobytes(), t
        _check_read(rv, hb, sig, **kw)
        one.drop()
    for hb in batch:
        hb.drop()


@pytest.mark.parametrize("mode", ["joint", "raw", "event"])
def test_decode_equals_the_padded_call_on_the_fetched_tables(rv, mode):
    b = _mk(rv, mode)
    sig = spi.synthetic_signal(rv, 66, 5)
    h = b.put_signal(sig, stride=2, max_raw_len=T_R, max_event_len=T_E)
    rows = h.windows[:16]
    assert rows.shape == (16, 4) and len({r.tobytes() for r in rows}) == 16
    raw, ev = rv.data_loader.expand_windows(h.fetch("raw_sc"), h.fetch("events_sc"), rows, T_R, T_E, 0.0)
    x = {"joint": (raw, ev), "raw": raw, "event": ev}[mode]
    for W in (1, 5):
        t, s = b.beam_search_prediction(x, W, L)
        want = (t.numpy().copy(), s.numpy().copy(), int(t.shape[1]))
        got = b.beam_search_windows(h.table(rows), W, L, T_r=T_R, T_e=T_E)
        assert _same(got, want), (mode, W)
        again = b.beam_search_windows(h.table(rows), W, L, T_r=T_R, T_e=T_E)
        assert _same(again, want), "same inputs, same bytes"
    assert want[2] > 2 and len({r.tobytes() for r in want[0]}) > 4, "the chunks decode to different calls"
    h.drop()
    b.close()


def test_basecall_many_with_device_prep(rv, bc):
    sigs = [spi.synthetic_signal(rv, 66, 5), spi.synthetic_signal(rv, 90, 9)]
    many = bc.basecall_many(sigs, stride=4, chunk_size=16, device_prep=True)
    for sig, got in zip(sigs, many):
        one = bc.basecall(sig, stride=4, chunk_size=16, device_prep=True)
        host = bc.basecall(sig, stride=4, chunk_size=16)
        assert got.seq == one.seq and got.probs.tobytes() == one.probs.tobytes() and got.chunks_num == one.chunks_num
        assert len(got.seq) > L - 1 and got.chunks_num > 5, "more bases than one chunk can call: a merged sequence"
        assert got.seq == host.seq and got.chunks_num == host.chunks_num, "the host path calls the same bases"
    assert int(bc.get_tensor("read_stats")[1]) == 0, "every read was dropped"


def test_put_while_a_ticket_is_in_flight_then_drop(rv, bc):
    sig = spi.synthetic_signal(rv, 66, 5)
    kw = dict(stride=2, max_raw_len=T_R, max_event_len=T_E)
    a = bc.put_signal(sig, **kw)
    table = a.table(a.windows[:12])
    want = bc.beam_search_windows(table, 5, L, T_r=T_R, T_e=T_E)
    ticket = bc.submit_windows(table, 5, L, T_r=T_R, T_e=T_E)
    b = bc.put_signal(spi.plateau_signal(2500), **kw)           # allowed with the ticket uncollected
    with pytest.raises(rv._capi.RavventHipError, match="RV_ESTATE"):
        a.drop()                                                # ... while the read the ticket uses cannot be dropped
    got = bc.collect(ticket)
    assert np.array_equal(np.asarray(got[0]), np.asarray(want[0])) and np.asarray(got[1]).tobytes() == np.asarray(want[1]).tobytes()
    _check_read(rv, b, spi.plateau_signal(2500), **kw)
    a.drop(); b.drop()
    assert int(bc.get_tensor("read_stats")[1]) == 0
