"""The chunker in window form (data_loader.prepare_windows / expand_windows) against the fixtures that pin prepare_snippets, and the
Phred mapping of Basecaller.basecall's result.  CPU only.

A window table must describe exactly the chunks the snippet cutter copies out: the same lengths, the same f32 values (fp64 scaling,
one cast), the same targets -- for labelled reads (the three fixtures: chunks_b has an event window longer than the 30 the padding
keeps) and for an unlabelled read, which is defined as prepare_snippets given the one label range that covers every event."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["chunks_a", "chunks_b", "chunks_c"]


def _fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=True)
    return z, z["signal"], z["label_ranges"], np.array(list(str(z["label_bases"]))), int(z["stride"])


def _slices(concat, lens):
    ends = np.cumsum(lens)
    return [concat[e - n:e] for n, e in zip(lens, ends)]


@pytest.mark.parametrize("name", NAMES)
def test_windows_reproduce_the_fixture(rv, name):
    dl = rv.data_loader
    z, sig, ranges, bases, stride = _fixture(name)
    w = dl.prepare_windows(sig, ranges, bases, stride)
    assert w.raw_sc.dtype == np.float32 and w.events_sc.dtype == np.float32 and w.windows.dtype == np.int32
    assert w.raw_sc.shape == (sig.shape[0],) and w.events_sc.ndim == 2 and w.events_sc.shape[1] == 5
    n = len(z["raw_lens"])
    assert w.windows.shape == (n, 4) and list(w.targets) == [str(t) for t in z["targets"]]
    # the lengths: the fixture's, cut where the padding cuts them (post-truncation)
    assert (w.windows[:, 1] == np.minimum(z["raw_lens"], dl.MAX_RAW_LEN)).all()
    assert (w.windows[:, 3] == np.minimum(z["ev_lens"], dl.MAX_EVENT_LEN)).all()
    assert (z["ev_lens"] > dl.MAX_EVENT_LEN).any() == (name == "chunks_b")
    # the values: fp64 -> f32 on both sides, untruncated (expanded to the longest window of the fixture)
    T_r, T_e = int(z["raw_lens"].max()), int(z["ev_lens"].max())
    full = w.windows.copy()
    full[:, 1], full[:, 3] = z["raw_lens"], z["ev_lens"]
    raw, ev = dl.expand_windows(w.raw_sc, w.events_sc, full, T_r, T_e, pad=0.0)
    for i, (r, e) in enumerate(zip(_slices(z["raw_concat"], z["raw_lens"]), _slices(z["ev_concat"], z["ev_lens"]))):
        assert raw[i, :len(r), 0].tobytes() == r.astype(np.float32).tobytes(), i
        assert ev[i, :len(e)].tobytes() == e.astype(np.float32).tobytes(), i
        assert not raw[i, len(r):].any() and not ev[i, len(e):].any(), i


@pytest.mark.parametrize("name", NAMES)
def test_expand_equals_the_padded_slab(rv, name):
    dl = rv.data_loader
    _, sig, ranges, bases, stride = _fixture(name)
    w = dl.prepare_windows(sig, ranges, bases, stride)
    raw, ev, _ = dl.snippets_to_slab(*dl.prepare_snippets(sig, ranges, bases, stride))
    xr, xe = dl.expand_windows(w.raw_sc, w.events_sc, w.windows, dl.MAX_RAW_LEN, dl.MAX_EVENT_LEN, dl.INPUT_PADDING)
    assert xr.dtype == raw.dtype and xr.shape == raw.shape and xr.tobytes() == raw.tobytes()
    assert xe.dtype == ev.dtype and xe.shape == ev.shape and xe.tobytes() == ev.tobytes()
    er, ee = w.expand()
    assert er.tobytes() == raw.tobytes() and ee.tobytes() == ev.tobytes()
    # a narrower padding cuts the same way pad_sequences does
    raw2, ev2, _ = dl.snippets_to_slab(*dl.prepare_snippets(sig, ranges, bases, stride), max_raw_len=150, max_event_len=20)
    xr2, xe2 = dl.expand_windows(w.raw_sc, w.events_sc, w.windows, 150, 20, dl.INPUT_PADDING)
    assert xr2.tobytes() == raw2.tobytes() and xe2.tobytes() == ev2.tobytes()


def _covering_range(rv, sig):
    from ravvent_basecaller_amd.event_detection import EventDetector
    dl = rv.data_loader
    st, ln, _, _ = EventDetector(window_length1=dl.ED_WINDOW_LENGTH_1, window_length2=dl.ED_WINDOW_LENGTH_2).run_arrays(np.asarray(sig))
    return np.array([[int(st[0]), int(st[-1] + ln[-1])]]), int(st[-1] + ln[-1])


@pytest.mark.parametrize("name,cut", [("chunks_a", 0), ("chunks_c", 0), ("chunks_b", 5)])
def test_unlabelled_read_is_the_single_covering_range(rv, name, cut):
    """prepare_windows(signal) == prepare_snippets with the label range [first event's start, last event's end); `cut` drops samples
    from the end of the signal until the last event ends before the last sample."""
    dl = rv.data_loader
    _, sig, _, _, stride = _fixture(name)
    sig = sig[:len(sig) - cut] if cut else sig
    rng, end = _covering_range(rv, sig)
    if cut:
        while end == len(sig):                  # make sure the case is the one the name says
            sig = sig[:-1]
            rng, end = _covering_range(rv, sig)
        assert end < len(sig)
    w = dl.prepare_windows(sig, stride=stride)
    assert w.targets is None and len(w) > 10
    labelled = dl.prepare_windows(sig, rng, np.array(["A"]), stride)
    assert np.array_equal(w.windows, labelled.windows)
    assert w.raw_sc.tobytes() == labelled.raw_sc.tobytes() and w.events_sc.tobytes() == labelled.events_sc.tobytes()
    raw, ev, _ = dl.snippets_to_slab(*dl.prepare_snippets(sig, rng, np.array(["A"]), stride))
    xr, xe = w.expand()
    assert xr.tobytes() == raw.tobytes() and xe.tobytes() == ev.tobytes()
    # every window lies inside its table
    assert (w.windows >= 0).all()
    assert (w.windows[:, 0] + w.windows[:, 1] <= w.raw_sc.shape[0]).all() and (w.windows[:, 2] + w.windows[:, 3] <= w.events_sc.shape[0]).all()


def test_phred_mapping_and_fastq():
    from ravvent_basecaller_amd.basecaller import BasecallResult, phred_qualities
    p = np.array([0.0, 0.9, 0.999, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0))], np.float32)
    q = phred_qualities(p)
    assert q.dtype == np.uint8 and q.tolist() == [0, 10, 30, 40, 40]
    assert phred_qualities(np.array([-0.5, 0.99995, 0.5])).tolist() == [0, 40, 3]
    res = BasecallResult("ACGTA", p, 3)
    assert res.qualities.tolist() == [0, 10, 30, 40, 40] and res.chunks_num == 3 and res.probs.dtype == np.float32
    lines = res.to_fastq("read_1").split("\n")
    assert lines[-1] == "" and len(lines) == 5
    name, seq, plus, qual = lines[:4]
    assert name == "@read_1" and seq == "ACGTA" and plus == "+" and len(qual) == len(seq)
    assert qual == "".join(chr(33 + int(x)) for x in q)
    empty = BasecallResult("", np.zeros(0, np.float32), 0).to_fastq("e").split("\n")
    assert empty[:4] == ["@e", "", "+", ""]
