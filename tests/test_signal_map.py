"""CPU side of the signal map: the new symbols, the merger's provenance, the position formulas of
Basecaller.basecall(..., moves=True) on hand-worked numbers, and the fp64 statement of the forced moves (tests/signal_map_reference.py)
that tests/test_signal_map_gpu.py holds rv_teacher_forced_moves to.  Runs without a GPU."""
import os
import re

import numpy as np
import pytest

import moves_reference as M
import signal_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared_and_bound(rv):
    hdr = open(os.path.join(ROOT, "include", "ravvent_hip.h")).read()
    mhdr = open(os.path.join(ROOT, "include", "ravvent_merge.h")).read()
    bound = {n: args for n, _, args in rv._capi.SYMBOLS}
    for name, nargs, h in (("rv_beam_search_calls_moves", 14, hdr), ("rv_beam_search_windows_calls_moves", 13, hdr),
                           ("rv_beam_search_submit_windows_calls_moves", 9, hdr), ("rv_beam_search_collect_calls_moves", 7, hdr),
                           ("rv_teacher_forced_moves", 13, hdr), ("rv_teacher_forced_moves_dev", 13, hdr), ("rv_merger_sources", 5, mhdr)):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", h, re.M)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == nargs == len(bound[name]), name
    m = re.search(r"typedef struct RvCallMoves \{([^}]*)\} RvCallMoves;", hdr)
    fields = [f.split("*")[-1].strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == [n for n, _ in rv._capi.CRvCallMoves._fields_] == list(M.FIELDS)
    assert re.search(r"#define RV_ABI_VERSION 1\b", hdr), "adding entry points keeps the ABI version"
    for method in ("beam_search_calls_moves", "beam_search_windows_calls_moves", "collect_calls_moves", "align", "label_positions"):
        assert callable(getattr(rv.Basecaller, method))
    import inspect
    assert "moves" in inspect.signature(rv.Basecaller.basecall).parameters and "moves" in inspect.signature(rv.Basecaller.basecall_many).parameters
    assert "sources" in inspect.signature(rv.merger.Merger.merge_arrays).parameters and callable(rv.merger.StreamingMerger.sources)
    r = rv.basecaller.BasecallResult("AC", [0.9, 0.5], 1)
    assert r.positions is None and r.raw_mass is None and r.event_mass is None and r.source_chunk is None and r.source_index is None


# ---------------------------------------------------------------------------------------------- merger provenance
STRIDE = 63


def _chunks_of(rng, kind, n_chunks):
    """Chunk calls of one synthetic read: windows of a true sequence, each with its own errors, so that neighbours overlap."""
    if kind == "random":
        truth = "".join(rng.choice(list("ACGT"), 40 + 22 * n_chunks))
    elif kind == "repeat":
        unit = "".join(rng.choice(list("ACGT"), int(rng.integers(1, 4))))
        truth = (unit * 400)[:40 + 22 * n_chunks]
    else:                                          # low complexity with islands
        truth = "".join(rng.choice(list("AC"), 40 + 22 * n_chunks, p=[0.85, 0.15]))
    out = []
    for i in range(n_chunks):
        a = 22 * i + int(rng.integers(0, 4))
        s = list(truth[a:a + int(rng.integers(30, 60))])
        for k in range(len(s)):
            if rng.random() < 0.08:
                s[k] = str(rng.choice(list("ACGT")))
        if rng.random() < 0.3 and len(s) > 5:
            del s[int(rng.integers(0, len(s)))]
        out.append("".join(s))
    return out


def _arrays(rng, seqs):
    n = len(seqs)
    bases, probs = np.zeros((n, STRIDE), np.uint8), np.zeros((n, STRIDE), np.float32)
    lens = np.array([len(s) for s in seqs], np.int32)
    for i, s in enumerate(seqs):
        bases[i, :len(s)] = np.frombuffer(s.encode(), np.uint8)
        probs[i, :len(s)] = rng.uniform(0.05, 1.0, len(s)).astype(np.float32)
    return bases, probs, lens


def _check_sources(tag, bases, probs, lens, seq, pr, ck, ix):
    assert len(seq) == len(pr) == len(ck) == len(ix), tag
    assert ck.dtype == np.int32 and ix.dtype == np.int32, tag
    if not len(seq):
        return
    assert (ck >= 0).all() and (ck < len(lens)).all() and (ix >= 0).all() and (ix < lens[ck]).all(), (tag, "a pair outside its chunk's call")
    assert bases[ck, ix].tobytes().decode() == seq, (tag, "letters")
    assert probs[ck, ix].tobytes() == np.asarray(pr, np.float32).tobytes(), (tag, "probabilities")
    same = ck[1:] == ck[:-1]
    assert (ix[1:][same] > ix[:-1][same]).all(), (tag, "indices inside a run from one chunk")


@pytest.mark.parametrize("scores_id", [0, 1, 2])
def test_merger_sources(rv, scores_id):
    mg = rv.merger
    rng = np.random.default_rng(100 + scores_id)
    m = mg.Merger(scores_id)
    both_sides = multi = 0
    for r in range(120):
        kind = ("random", "repeat", "low")[r % 3]
        seqs = _chunks_of(rng, kind, int(rng.integers(2, 13)))
        bases, probs, lens = _arrays(rng, seqs)
        tag = (scores_id, r, kind)
        seq0, pr0 = m.merge_arrays(bases, probs, lens)
        seq, pr, ck, ix = m.merge_arrays(bases, probs, lens, sources=True)
        assert seq == seq0 and pr.tobytes() == pr0.tobytes(), (tag, "sources=True changed the merge")
        _check_sources(tag, bases, probs, lens, seq, pr, ck, ix)
        multi += len(set(ck.tolist())) >= 2
        # picks from both sides of one overlap: a base of chunk k behind a base of chunk k + 1
        both_sides += bool((np.diff(ck.astype(np.int64)) < 0).any())
        # streaming appends in two pieces: the same merge, the same sources, chunks counted over all appends
        cut = int(rng.integers(1, len(seqs)))
        sm = mg.StreamingMerger(scores_id)
        sm.append(bases[:cut], probs[:cut], lens[:cut])
        sm.append(bases[cut:], probs[cut:], lens[cut:])
        s2, p2 = sm.result()
        c2, i2 = sm.sources()
        sm.close()
        assert s2 == seq and p2.tobytes() == pr.tobytes() and np.array_equal(c2, ck) and np.array_equal(i2, ix), (tag, "two appends", cut)
    print(f"scores_id {scores_id}: reads with bases of several chunks {multi}, with picks from both sides of an overlap {both_sides}")
    assert multi >= 60 and both_sides >= 5, (multi, both_sides)


@pytest.mark.parametrize("scores_id", [0, 1, 2])
def test_merger_sources_replace_and_early_stop(rv, scores_id):
    mg = rv.merger
    rng = np.random.default_rng(7)
    m = mg.Merger(scores_id)
    body = _chunks_of(rng, "random", 4)
    # while nothing has merged, a chunk that aligns nowhere REPLACES the read so far: A.. then C.. share no letter
    seqs = ["A" * 30, "C" * 31] + ["C" * 5 + body[0]] + body[1:]
    bases, probs, lens = _arrays(rng, seqs)
    seq, pr, ck, ix = m.merge_arrays(bases, probs, lens, sources=True)
    assert (seq, pr.tobytes()) == (lambda s, p: (s, p.tobytes()))(*m.merge_arrays(bases, probs, lens))
    _check_sources((scores_id, "replace"), bases, probs, lens, seq, pr, ck, ix)
    assert ck.min() == 1 and ix[0] == 0 and ck[0] == 1, "chunk 0 was replaced by chunk 1 before the first merge"
    assert ck.max() >= 3, "the merge went on behind the replacement"
    only = m.merge_arrays(bases[:2], probs[:2], lens[:2], sources=True)
    assert only[0] == "C" * 31 and (only[2] == 1).all() and np.array_equal(only[3], np.arange(31))
    # after a merge, a chunk that aligns nowhere ENDS the read: what follows is ignored
    ac = ["".join(rng.choice(list("AC"), 70))]
    seqs = [ac[0][:45], ac[0][25:70], "G" * 30, ac[0][40:70], "T" * 12]
    bases, probs, lens = _arrays(rng, seqs)
    seq, pr, ck, ix = m.merge_arrays(bases, probs, lens, sources=True)
    first_two = m.merge_arrays(bases[:2], probs[:2], lens[:2], sources=True)
    assert seq == first_two[0] and pr.tobytes() == first_two[1].tobytes() and np.array_equal(ck, first_two[2]) and np.array_equal(ix, first_two[3])
    assert set(ck.tolist()) == {0, 1} and "G" not in seq, "the early stop"
    _check_sources((scores_id, "stop"), bases, probs, lens, seq, pr, ck, ix)
    # the chunk counter runs over every appended chunk, the ignored ones included
    sm = mg.StreamingMerger(scores_id)
    sm.append(bases[:3], probs[:3], lens[:3])
    sm.append(bases[3:], probs[3:], lens[3:])
    assert np.array_equal(sm.sources()[0], ck) and sm.result()[0] == seq
    sm.close()
    # an empty result
    e = m.merge_arrays(np.zeros((1, 4), np.uint8), np.zeros((1, 4), np.float32), np.zeros(1, np.int32), sources=True)
    assert e[0] == "" and len(e[2]) == 0 and len(e[3]) == 0


# ---------------------------------------------------------------------------------------------- position formulas
def test_position_formulas_on_hand_worked_numbers(rv):
    bcm = rv.basecaller
    nan = float("nan")
    # raw: raw_start + raw_pos
    got = bcm.raw_position_estimate([100, 0, 7], np.array([2.5, 0.0, nan], np.float32))
    assert got.dtype == np.float64 and got[0] == 102.5 and got[1] == 0.0 and np.isnan(got[2])
    assert bcm.raw_position_estimate([100], [2.5], offset=10)[0] == 112.5
    # events: starts 0, 10, 30, 36 and lengths 10, 20, 6, 4 -> centres 5, 20, 33, 38
    st, ln = np.array([0, 10, 30, 36]), np.array([10, 20, 6, 4])
    f = lambda es, ep: bcm.event_position_estimate(es, np.asarray(ep, np.float32), st, ln)
    assert f([0], [0.0])[0] == 5.0                      # the first event's centre
    assert f([0], [0.5])[0] == 12.5                     # half way to the second: 5 + 0.5 (20 - 5)
    assert f([1], [0.25])[0] == 23.25                   # e = 1.25: 20 + 0.25 (33 - 20)
    assert f([2], [1.0])[0] == 38.0                     # e = 3: the last event, its centre
    assert f([3], [0.75])[0] == 38.0                    # e = 3.75 inside the last event: c_min(i+1, E-1) = c_i
    assert f([3], [5.0])[0] == 38.0                     # beyond the read's events: i clipped to E - 1
    assert f([0], [-1.0])[0] == 5.0 + (-1.0 - 0) * 15   # e = -1 (a segment without weight): as computed, i clipped to 0
    assert np.isnan(f([1], [nan])[0])
    assert np.isnan(bcm.event_position_estimate([0], [0.5], np.zeros(0), np.zeros(0))[0])        # a read without events
    # the choice: raw mode raw, event mode events, joint mode raw where raw_mass >= event_mass
    args = dict(raw_start=np.array([100, 100, 100, 100]), event_start=np.array([1, 1, 1, 1]),
                raw_pos=np.array([2.5, 2.5, 2.5, nan], np.float32), raw_mass=np.array([0.6, 0.5, 0.2, nan], np.float32),
                event_pos=np.array([0.25, 0.25, 0.25, nan], np.float32), event_mass=np.array([0.4, 0.5, 0.8, nan], np.float32),
                ev_starts=st, ev_lengths=ln)
    raw, ev, joint = (bcm.signal_positions(m, **args) for m in ("raw", "event", "joint"))
    assert raw[:3].tolist() == [102.5] * 3 and np.isnan(raw[3])
    assert ev[:3].tolist() == [23.25] * 3 and np.isnan(ev[3])
    assert joint[:3].tolist() == [102.5, 102.5, 23.25] and np.isnan(joint[3])
    # positions_tsv: index, letter, position, Phred
    r = bcm.BasecallResult("ACG", [0.9, 0.99, 0.5], 2, positions=np.array([1.5, nan, 20.0]), raw_mass=np.zeros(3, np.float32),
                           event_mass=np.zeros(3, np.float32), source_chunk=np.zeros(3, np.int32), source_index=np.arange(3, dtype=np.int32))
    assert r.positions_tsv("read1") == "# read1\n0\tA\t1.500\t10\n1\tC\tnan\t20\n2\tG\t20.000\t3\n"
    with pytest.raises(ValueError):
        bcm.BasecallResult("A", [0.5], 1).positions_tsv("x")


# ---------------------------------------------------------------------------------------------- the forced-moves reference
@pytest.mark.parametrize("family", ["bilstm", "bigru"])
def test_forced_reference_fed_the_greedy_ids_is_the_greedy_decode(rv, oracle, family):
    """Fed [start | the fp64 greedy search's own ids], the forced loop's alignments -- hence its records -- are the greedy search's."""
    import gru_reference as G
    raw, ev, _ = rv.synthetic.make_slab(3, 14, 5, seed=4)
    raw[2], ev[2] = 0.0, 0.0                                     # a chunk that is padding from end to end: NaN alignments
    for attention, depth in (("luong", 1), ("bahdanau", 1), ("luong", 2)):
        cfg = rv.RvConfig(enc_units=16, dec_units=16, enc_depth=2, dec_depth=depth, attention=attention, rnn=family)
        flat = rv.weights.init_weights(cfg, seed=5, gain=2.0)
        flat["b_fc"][cfg.end_token] -= 4.0
        w = rv.weights.flat_to_nested(cfg, flat)
        L, T_r = 7, 14
        ref = G if family == "bigru" else oracle
        taps = {}
        ids, _ = ref.greedy_search(w, cfg.oracle_cfg(), raw, ev, L, taps=taps)
        assert ids[:2].shape[1] == L - 1
        target = np.concatenate([np.full((3, 1), cfg.start_token, np.int32), ids], axis=1)
        target[2, 1:] = 3                                        # (the argmax of its NaN logits is id 0, the padding token: give it letters)
        mv, al = R.forced_moves(oracle, w, cfg.oracle_cfg(), raw, ev, target, T_r, cfg.pad_token, gru=G if family == "bigru" else None)
        want = np.transpose(taps["step_alignments"], (1, 0, 2))
        assert np.array_equal(al[:2], want[:2]) and np.isnan(al[2]).all() and np.isnan(want[2]).all(), (family, attention, depth)
        rec = M.records(want, T_r)
        lab = ids[:2] != cfg.pad_token                           # (a greedy id may be the padding token: its column holds the fill values)
        assert lab.sum() >= 5, "labels to compare"
        assert np.array_equal(mv["raw_mass"][:2][lab], rec[:2, :, 0][lab]) and np.array_equal(mv["peak"][:2][lab], rec[:2, :, 5].astype(np.int32)[lab])
        assert np.allclose((mv["raw_mass"][:2] + mv["event_mass"][:2])[lab], 1.0, atol=1e-12)
        live = lab & (rec[:2, :, 0] > 0)
        assert live.any() and (mv["raw_pos"][:2][live] == (rec[:2, :, 1] / np.where(rec[:2, :, 0] > 0, rec[:2, :, 0], 1))[live]).all()
        assert (mv["raw_pos"][:2][lab & ~live] == -1).all() and (mv["raw_pos"][:2][~lab] == -1).all() and (mv["raw_mass"][:2][~lab] == 0).all()
        assert np.isnan(mv["raw_mass"][2]).all() and np.isnan(mv["event_pos"][2]).all() and (mv["peak"][2] == -1).all(), "the NaN rule"
        # a padding label: the fill values in its column, whatever the step computed
        padded = target.copy()
        padded[0, 4:] = cfg.pad_token
        pm, _ = R.forced_moves(oracle, w, cfg.oracle_cfg(), raw, ev, padded, T_r, cfg.pad_token, gru=G if family == "bigru" else None)
        assert (pm["raw_pos"][0, 3:] == -1).all() and (pm["raw_mass"][0, 3:] == 0).all() and (pm["peak"][0, 3:] == -1).all()
        assert np.array_equal(pm["raw_pos"][0, :3], mv["raw_pos"][0, :3])

