"""The signal map in numpy: what the forced moves must be.

forced_alignments():  Decoder.call under TrainingSampler with the alignments kept -- the loop of test_teacher_forced._forced_loop over
                      oracle.attention_step, whose third result is the step's alignments; for a BiGRU model the taps of
                      gru_reference.greedy_search(forced=...).  -> [B, L-1, T_m] in the dtype asked for.
forced_moves():       those alignments through moves_reference.records (one beam row, W = 1), the quotients of
                      moves_reference.finalize, and the fill values where the label of a column, target[b, t + 1], is the padding token.
"""
import numpy as np

import moves_reference as M

FILL = dict(raw_pos=-1, raw_mass=0, event_pos=-1, event_mass=0, peak=-1, peak_weight=0)


def forced_alignments(oracle, w, cfg, raw, ev, target, dtype=np.float64, gru=None):
    target = np.asarray(target)
    if gru is not None:
        taps = {}
        gru.greedy_search(w, cfg, raw, ev, target.shape[1], dtype=dtype, taps=taps, forced=target)
        al = taps["step_alignments"]
        return np.transpose(al, (1, 0, 2)) if al is not None else np.zeros((target.shape[0], 0, 0), dtype)
    enc_out, mask = oracle.encode_input(w, raw, ev, cfg["mode"], cfg.get("padding_value", 0.0), dtype)
    keys, values = oracle.setup_memory(w, enc_out, mask, dtype)
    B, d = enc_out.shape[0], np.asarray(w["W_att"]).shape[1]
    att = np.zeros((B, d), dtype)
    states = [(np.zeros((B, d), dtype), np.zeros((B, d), dtype)) for _ in w["dec_cells"]]
    out = []
    for s in range(target.shape[1] - 1):
        _, att, alpha, states = oracle.attention_step(w, target[:, s], att, states, keys, values, mask, cfg["attention_type"], dtype)
        out.append(alpha)
    return np.stack(out, axis=1) if out else np.zeros((B, 0, enc_out.shape[1]), dtype)


def moves_of_alignments(alignments, T_r, labels=None, pad=0):
    """alignments [B, S, T_m] -> dict of the six outputs [B, S] in fp64 (peak int32); labels [B, S]: fill where labels == pad."""
    rec = M.records(alignments, T_r)
    out = dict(raw_mass=rec[..., 0].copy(), event_mass=rec[..., 2].copy(), peak_weight=rec[..., 4].copy(), peak=rec[..., 5].astype(np.int32),
               raw_pos=M._quot(rec[..., 1], rec[..., 0], np.float64), event_pos=M._quot(rec[..., 3], rec[..., 2], np.float64))
    if labels is not None:
        for k in out:
            out[k][np.asarray(labels) == pad] = FILL[k]
    return out


def forced_moves(oracle, w, cfg, raw, ev, target, T_r, pad=0, gru=None):
    al = forced_alignments(oracle, w, cfg, raw, ev, target, np.float64, gru)
    return moves_of_alignments(al, T_r, np.asarray(target)[:, 1:], pad), al

