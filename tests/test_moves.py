"""The moves, on the CPU: the numpy statement (tests/moves_reference.py) on a case worked by hand, its fill rules, the cut to letters
(Basecaller.base_positions), and the oracle's fp64 alignments at the Luong shape of tests/test_moves_gpu.py."""
import numpy as np
import pytest

import moves_reference as M

END = 1


def _micro():
    """S = 2, W = 2, T_r = 3, T_e = 1, no end token, lengths 2: a case small enough to work by hand (the parent-row rule)."""
    al = np.array([[[[.5, .25, .25, 0], [0, 0, .5, .5]]],            # step 0: rows 0, 1
                   [[[0, 0, 1, 0], [.25, .25, .25, .25]]]])          # step 1
    ids = np.array([[[3, 4]], [[5, 6]]])
    par = np.array([[[0, 0]], [[1, 0]]])
    ln = np.array([[2, 2]])
    return al, ids, par, ln


def test_hand_worked_micro_case():
    al, ids, par, ln = _micro()
    o = M.moves_reference(al, ids, par, ln, 3, END)
    g = lambda k, w, t: float(o[k][0, t, w])
    # hypothesis 0, column 1: slot 0 of step 1 came from row 1
    assert (g("raw_mass", 0, 1), g("raw_pos", 0, 1), g("event_mass", 0, 1), g("event_pos", 0, 1)) == (.75, 1.0, .25, 0.0)
    assert (int(o["peak"][0, 1, 0]), g("peak_weight", 0, 1)) == (0, .25)
    # hypothesis 0, column 0: its back-trace passes slot 1 of step 0, which came from row 0
    assert (g("raw_mass", 0, 0), g("raw_pos", 0, 0), g("event_mass", 0, 0), g("event_pos", 0, 0)) == (1.0, .75, 0.0, -1.0)
    assert (int(o["peak"][0, 0, 0]), g("peak_weight", 0, 0)) == (0, .5)
    # hypothesis 1, column 1: from row 0
    assert (g("raw_pos", 1, 1), int(o["peak"][0, 1, 1]), g("peak_weight", 1, 1)) == (2.0, 2, 1.0)
    # hypothesis 1, column 0: as hypothesis 0's
    for k in M.FIELDS:
        assert o[k][0, 0, 1] == o[k][0, 0, 0], k
    # indexing the records by slot instead of parent gives 2.0 and 2.0 for hypothesis 0
    rec = M.records(al, 3)
    slot, _ = M.slots(par, ln)
    by_slot = [rec[t, 0, slot[0, t, 0], 1] / rec[t, 0, slot[0, t, 0], 0] for t in (0, 1)]
    assert by_slot == [2.0, 2.0] and [g("raw_pos", 0, 0), g("raw_pos", 0, 1)] != by_slot


def test_fills_past_an_end_token_and_a_nan_row():
    # S = 3, W = 2: hypothesis 0 ends at its second token (length 2), hypothesis 1 runs on (length 3)
    rng = np.random.default_rng(0)
    al = rng.random((3, 2, 2, 5))
    al /= al.sum(-1, keepdims=True)
    al[:, 1] = np.nan                                   # chunk 1: padding from end to end
    ids = np.array([[[3, 4], [3, 4]], [[END, 5], [5, 5]], [[END, 6], [6, 6]]])
    par = np.array([[[0, 0], [0, 0]], [[0, 1], [0, 1]], [[0, 1], [0, 1]]])
    ln = M.tfa_lengths(ids, par, END)
    assert ln.tolist() == [[2, 3], [3, 3]]
    o = M.moves_reference(al, ids, par, ln, 4, END)
    assert o["raw_pos"][0, 2, 0] == -1 and o["event_pos"][0, 2, 0] == -1 and o["peak"][0, 2, 0] == -1
    assert o["raw_mass"][0, 2, 0] == 0 and o["event_mass"][0, 2, 0] == 0 and o["peak_weight"][0, 2, 0] == 0
    assert (o["raw_mass"][0, :2, 0] > 0).all() and (o["raw_mass"][0, :, 1] > 0).all() and (o["peak"][0, :, 1] >= 0).all()
    for k in ("raw_pos", "raw_mass", "event_pos", "event_mass", "peak_weight"):
        assert np.isnan(o[k][1]).all(), k
    assert (o["peak"][1] == -1).all()
    # raw mode (T_r = T_m): no event mass, position -1; event mode (T_r = 0): the same for the raw segment
    o = M.moves_reference(al[:, :1], ids[:, :1], par[:, :1], ln[:1], 5, END)
    assert (o["event_mass"] == 0).all() and (o["event_pos"] == -1).all() and np.allclose(o["raw_mass"][0, :, 1], 1)
    o = M.moves_reference(al[:, :1], ids[:, :1], par[:, :1], ln[:1], 0, END)
    assert (o["raw_mass"] == 0).all() and (o["raw_pos"] == -1).all() and np.allclose(o["event_mass"][0, :, 1], 1)


def test_base_positions_follow_the_strings(rv):
    bc = object.__new__(rv.Basecaller)                  # the two helpers need the tokenizer only
    bc.tokenizer = rv.data_loader.nuc_tk
    tok = np.array([[2, 3, 4, 1, 0, 0], [3, 1, 1, 1, 0, 0], [1, 1, 1, 1, 0, 0], [6, 5, 2, 4, 3, 1]], np.int32)   # '$' = 2, '^' = 1, '' = 0
    pos = np.arange(tok.size, dtype=np.float32).reshape(tok.shape)
    strings = bc.tokens_to_nuc_sequences(tok)
    got = bc.base_positions(tok, pos)
    assert strings == ["AC", "A", "", "TGCA"]
    assert [len(g) for g in got] == [len(s) for s in strings]
    assert [g.tolist() for g in got] == [[1.0, 2.0], [6.0], [], [18.0, 19.0, 21.0, 22.0]]
    import torch
    got_t = bc.base_positions(torch.from_numpy(tok), torch.from_numpy(pos))
    assert all((a == b).all() for a, b in zip(got, got_t))
    with pytest.raises(ValueError):
        bc.base_positions(tok, pos[:, :3])


def test_oracle_positions_lie_inside_their_segments(rv, oracle):
    TR, TE, L, W = 40, 8, 14, 5                         # shape A of tests/test_moves_gpu.py, Luong with one cell, its seeds (1, 1)
    from test_kernel_forms_gpu import _slab
    cfg = rv.RvConfig(mode="joint", attention="luong", dec_depth=1, max_batch=6, max_raw_len=TR, max_event_len=TE, max_output_len=L)
    flat = rv.weights.init_weights(cfg, seed=1, gain=1.5)
    flat["b_fc"][cfg.end_token] = -0.02
    raw, ev = _slab("joint", TR, TE, seed=1)
    taps = {}
    oracle.beam_search(rv.weights.flat_to_nested(cfg, flat), cfg.oracle_cfg(), raw, ev, W, L, dtype=np.float64, taps=taps)
    o = M.moves_reference(taps["step_alignments"], taps["step_ids"], taps["parent_ids"], taps["lengths"], TR, cfg.end_token)
    live = np.arange(o["peak"].shape[1])[None, :, None] < taps["lengths"][:, None, :]
    assert live.any() and (o["peak"][live] >= 0).all() and (o["peak"][live] < TR + TE).all()
    assert (o["peak"][~live] == -1).all() and (o["raw_mass"][~live] == 0).all() and (o["raw_pos"][~live] == -1).all()
    for seg, n in (("raw", TR), ("event", TE)):
        mass, pos = o[seg + "_mass"], o[seg + "_pos"]
        has = live & (mass > 0)
        assert has.any(), seg
        assert np.isfinite(pos[has]).all() and (pos[has] >= 0).all() and (pos[has] < n).all(), seg
        assert (pos[live & (mass == 0)] == -1).all(), seg
    assert np.allclose((o["raw_mass"] + o["event_mass"])[live], 1.0, atol=1e-12)
