"""Stitching by signal position on the host alone: the numpy statement of the rule (tests/stitch_reference.py)
against a base-by-base loop, the property that makes the rule worth having, and the call forms that must not move."""
import inspect

import numpy as np
import pytest

import stitch_reference as R


def _random_read(rng, mode, n, stride):
    """Window rows and call tables of one read with everything the rule branches on: lengths 0 .. stride and beyond, NaN values,
    positions far outside every interval, equal masses, event positions on integers and past the last event."""
    E = int(rng.integers(0, 40))
    ev_len = rng.integers(1, 30, E).astype(np.int64)
    ev_start = np.concatenate([[0], np.cumsum(ev_len)[:-1]]).astype(np.int64) if E else np.zeros(0, np.int64)
    a = np.sort(rng.integers(0, 400, n))
    win = np.stack([a, rng.integers(0, 200, n), rng.integers(0, max(E, 1), n), rng.integers(0, 30, n)], axis=1).astype(np.int32)
    f = lambda lo, hi: rng.uniform(lo, hi, (n, stride)).astype(np.float32)
    raw_pos, event_pos = f(-20, 220), np.where(rng.random((n, stride)) < 0.3, np.floor(f(-2, 45)), f(-2, 45)).astype(np.float32)
    raw_mass, event_mass = f(0, 1), f(0, 1)
    event_mass[rng.random((n, stride)) < 0.2] = raw_mass[0, 0] if n and stride else 0
    raw_mass[rng.random((n, stride)) < 0.2] = raw_mass[0, 0] if n and stride else 0
    for arr in (raw_pos, event_pos, raw_mass, event_mass):
        arr[rng.random((n, stride)) < 0.05] = np.nan
    lengths = rng.integers(-1, stride + 3, n).astype(np.int32)
    bases = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n, stride))
    return win, bases, f(0, 1), lengths, raw_pos, raw_mass, event_pos, event_mass, ev_start, ev_len


@pytest.mark.parametrize("mode", ["raw", "event", "joint"])
def test_reference_against_loop(mode):
    rng = np.random.default_rng({"raw": 1, "event": 2, "joint": 3}[mode])
    kept = 0
    for n, stride in [(0, 5), (1, 1), (1, 7), (2, 3), (5, 0), (9, 11), (17, 6), (30, 13)]:
        for _ in range(8):
            args = _random_read(rng, mode, n, stride)
            got, want = R.stitch_read(mode, *args), R.stitch_read_loop(mode, *args)
            for k, g, w in zip(R.FIELDS, got, want):
                assert R.same_bits(g, w), (mode, n, stride, k)
            kept += len(got[0])
            # each kept base names a cell of its chunk below the chunk's length; the chunks come in order
            ck, ix = got[5], got[6]
            assert (np.diff(ck) >= 0).all() and (ix < np.clip(args[3], 0, stride)[ck]).all()
    assert kept > 100, ("vacuous", kept)


def test_multi_read_offsets():
    rng = np.random.default_rng(5)
    reads = [_random_read(rng, "joint", n, 6) for n in (4, 0, 7)]
    table = np.concatenate([np.column_stack([np.full(len(r[0]), i, np.int32), r[0]]) for i, r in enumerate(reads)])
    cat = lambda j: np.concatenate([r[j] for r in reads])
    rows = np.array([0, 4, 4, 11])
    out, offs = R.stitch("joint", table, rows, cat(1), cat(2), cat(3), cat(4), cat(5), cat(6), cat(7), [(r[8], r[9]) for r in reads])
    assert offs[0] == 0 and offs[1] == offs[2] and offs[3] == len(out[0])
    for i, r in enumerate(reads):
        one = R.stitch_read("joint", *r)
        for k, g, w in zip(R.FIELDS, out, one):
            assert R.same_bits(g[offs[i]:offs[i + 1]], w), (i, k)


def test_stitched_read_is_the_truth():
    """What the rule is for.  A synthetic read (stitch_reference.synthetic_read): bases 5-14 samples apart; windows of 150-300 samples
    that start every 20-79 samples, the last start before N - T/2; a chunk's call is the bases inside its window, with the letters
    within 12 samples of a window edge (other than the read's own) corrupted; every reported position is the true one plus one noise
    value per base, |noise| < 2.4, THE SAME IN EVERY CHUNK.  Then the stitched read is the truth, letter for letter: a chunk owns
    the signal to half way between its centre and its neighbours', which lies more than 12 + 2.4 samples inside its window, and with
    one position per base every base falls into exactly one chunk's interval.  300 reads, 0 failures.

    With the noise drawn independently per chunk this fails (291 of the same 300 reads): a base within the noise of a cut can lie
    below the cut in the later chunk and above it in the earlier one, or the other way round, and is then owned by neither or by
    both.  That is the double-ownership caveat of DESIGN.md section 19; the rule is exact about positions, not about the model."""
    none = np.zeros(0, np.int64)
    corrupted = 0
    for seed in range(300):
        d = R.synthetic_read(seed)
        out = R.stitch_read("raw", d["windows"], d["bases"], d["probs"], d["lengths"], d["raw_pos"], d["raw_mass"], d["event_pos"],
                            d["event_mass"], none, none)
        assert out[0].tobytes() == d["truth"].tobytes(), seed
        assert len(d["windows"]) >= 2
        corrupted += int((d["bases"] == ord("N")).sum())
    assert corrupted > 10000, ("the calls hold no corrupted letters to leave out", corrupted)


def test_call_forms(rv):
    """put_read and basecall keep their old positional forms; what is new comes behind them with defaults that change nothing."""
    names = lambda f: list(inspect.signature(f).parameters)
    B = rv.Basecaller
    assert names(B.put_read) == ["self", "raw_sc", "events_sc", "event_starts", "event_lengths"]
    p = inspect.signature(B.put_read).parameters
    assert p["event_starts"].default is None and p["event_lengths"].default is None
    old = ["self", "signal", "stride", "beam_width", "max_output_len", "chunk_size", "device_prep", "moves"]
    assert names(B.basecall) == old + ["merge"]
    assert names(B.basecall_many) == ["self", "signals"] + old[2:] + ["merge"]
    for f in (B.basecall, B.basecall_many):
        q = inspect.signature(f).parameters
        assert q["merge"].default == "align" and q["moves"].default is False and q["device_prep"].default is False
        assert (q["stride"].default, q["beam_width"].default, q["max_output_len"].default, q["chunk_size"].default) == (6, 5, None, 1024)
    assert callable(B.stitch_calls)
    for name in ("rv_stitch_calls", "rv_read_put_events", "rv_stitch_open", "rv_stitch_close", "rv_beam_search_submit_windows_stitch",
                 "rv_beam_search_collect_stitch", "rv_stitch_run"):
        assert name in [s[0] for s in rv._capi.SYMBOLS], name
