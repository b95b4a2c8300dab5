"""Host side of device signal preparation (CPU): the closed form of the chunk ranges against the chunker's loop,
the refusal of signals the device path cannot take exactly, and the inputs of tests/test_signal_prep_gpu.py, proven here to contain
what they are there for."""
import os

import numpy as np
import pytest

import signal_prep_inputs as spi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _same_ranges(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["chunks_a", "chunks_b", "chunks_c"])
def test_closed_form_on_the_chunk_fixtures(rv, name):
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=True)
    dl = rv.data_loader
    lens, stride = g["fit_lens"], int(g["stride"])
    got = dl.fitting_event_ranges_closed_form(lens, stride)
    assert _same_ranges(got, dl.compute_fitting_event_ranges(lens, stride))
    assert np.array_equal(got, g["fit_ranges"]), "the reference's own ranges"
    for s, mx in ((1, 200), (4, 200), (6, 20), (7, 55), (len(lens) + 3, 200)):
        assert _same_ranges(dl.fitting_event_ranges_closed_form(lens, s, mx), dl.compute_fitting_event_ranges(lens, s, mx)), (s, mx)


def test_closed_form_on_random_lengths(rv):
    dl = rv.data_loader
    rng = np.random.default_rng(17)
    oversized = 0
    for _ in range(4000):
        E = int(rng.integers(1, 70))
        lens = rng.integers(1, 1 + int(rng.integers(2, 90)), E)
        stride, mx = int(rng.integers(1, E + 4)), int(rng.integers(4, 130))
        want = dl.compute_fitting_event_ranges(lens, stride, mx)
        assert _same_ranges(dl.fitting_event_ranges_closed_form(lens, stride, mx), want), (lens, stride, mx)
        oversized += int(lens.max() > mx)
    assert oversized > 500, "events longer than the window are among the cases"


def test_closed_form_keeps_the_quirks(rv):
    dl = rv.data_loader
    loop, closed = dl.compute_fitting_event_ranges, dl.fitting_event_ranges_closed_form

    def both(lens, stride, mx):
        a = loop(np.array(lens), stride, mx)
        assert _same_ranges(closed(np.array(lens), stride, mx), a), (lens, stride, mx)
        return a

    # an oversized first event: no windows at all, although later chunks would fit
    assert both([30, 5, 5, 5, 5, 5, 5, 5, 5, 5], 2, 20).size == 0
    # an oversized event later: the chunk that starts on it has length zero (its end is its own start)
    a = both([5, 5, 30, 5, 5, 5, 5, 5, 5, 5, 5, 5], 2, 20)
    assert [2, 2] in a.tolist() and a.shape[0] > 2
    # the tail fits: the table ends at the first chunk whose remaining events stay inside the window
    a = both([5] * 12, 2, 20)
    assert a.tolist() == [[0, 4], [2, 6], [4, 8], [6, 10]], "chunks from event 8 on would fit whole: they are not made"
    # stride 1 and a stride beyond the number of events
    assert both([5] * 12, 1, 20).shape[0] == 8
    assert both([5] * 12, 13, 20).tolist() == [[0, 4]]
    assert both([5] * 3, 13, 20).size == 0
    assert closed(np.zeros(0, np.int64), 6, 200).size == 0


def test_signals_the_device_path_cannot_take_are_refused(rv):
    conv = rv.Basecaller._signal_int16
    assert conv(np.array([1.0, -3.0, 32767.0])).dtype == np.int16
    assert np.array_equal(conv(np.array([5, -32768, 32767], np.int64)), np.array([5, -32768, 32767], np.int16))
    assert conv(np.zeros(0)).shape == (0,)
    for bad in (np.array([1.0, 2.5]), np.array([1.0, np.nan]), np.array([0, 32768]), np.array([-32769, 0]), np.array([1e9])):
        with pytest.raises(ValueError, match="host path"):
            conv(bad)


# ---- the inputs of the GPU tests
def test_flat_read_has_the_single_wrapped_event(rv):
    det = rv.event_detection.EventDetector(6, 9)
    assert [tuple(e[:2]) for e in det.run(spi.flat_signal())] == [(0, 2)], "the start-up reads of the wrapped ring indices"
    rw = rv.data_loader.prepare_windows(spi.flat_signal())
    assert not rw.raw_sc.any() and len(rw) == 0, "a zero deviation scales by 1; one event of 2 samples fits: no window"


def test_one_event_read(rv):
    sig = spi.one_event_signal()
    assert len(set(sig.tolist())) > 3
    rw = rv.data_loader.prepare_windows(sig)
    assert rw.events_sc.shape == (1, 5) and not rw.events_sc.any() and rw.raw_sc.any()


def test_zero_length_window_read(rv):
    sig = spi.synthetic_signal(rv, 1500, 11)
    w = rv.data_loader.prepare_windows(sig, stride=6, max_raw_len=20).windows
    assert np.any((w[:, 1] == 0) & (w[:, 3] == 0)), "an event longer than max_raw_len starts a chunk: both windows are empty"
    assert np.any(w[:, 1] > 0) and w[:, 1].max() <= 20 and w.shape[0] > 200
    w3 = rv.data_loader.prepare_windows(sig, stride=6, max_event_len=3).windows
    assert (w3[:, 3] == 3).all() and w3.shape[0] > 200, "max_event_len 3 clips every chunk"


def test_sweep_signals_reach_the_limits(rv):
    assert int(np.abs(spi.plateau_signal(64).astype(np.int64)).min()) == 32767
    n = spi.MAX_SAMPLES
    assert n * 32767 ** 2 < 2 ** 53 < 4 * n * 32768 ** 2, "2^22 full-amplitude samples: the sum of x^2 is exact in fp64, not far below the limit"
    det = rv.event_detection.EventDetector(6, 9)
    for n in (30, 70, 257):
        for sig in (spi.step_signal(n), spi.plateau_signal(n)):
            assert len(det.run_arrays(sig)[0]) >= 2
    assert set(range(0, 71)) <= set(spi.LENGTHS) and {255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65537} <= set(spi.LENGTHS)
