"""The moves in numpy fp64: DESIGN.md section 12 restated from the alignments of every step.

records():  step_alignments [S,B,W,T_m] -> step_moves [S,B,W,6] (raw_mass, raw_m1, event_mass, event_m1, peak_weight, peak_t), one
            record per beam row as it is when the attention of the step runs.
finalize(): records + parent_ids + lengths -> the six outputs [B,S,W] of rv_beam_search_moves: the token hypothesis w holds at column
            t sits in slot p_t of the back-trace and was produced from row parent_ids[t][b][p_t] of step t.
moves_reference(): both, with the lengths checked against TFA's recurrence over step_ids / parent_ids.
"""
import numpy as np

FIELDS = ("raw_pos", "raw_mass", "event_pos", "event_mass", "peak", "peak_weight")


def records(step_alignments, T_r):
    a = np.asarray(step_alignments, np.float64)          # [..., T_m]: any leading shape
    Tm = a.shape[-1]
    t = np.arange(Tm, dtype=np.float64)
    rec = np.zeros(a.shape[:-1] + (6,))
    rec[..., 0] = a[..., :T_r].sum(-1)
    rec[..., 1] = (a[..., :T_r] * t[:T_r]).sum(-1)
    rec[..., 2] = a[..., T_r:].sum(-1)
    rec[..., 3] = (a[..., T_r:] * (t[T_r:] - T_r)).sum(-1)
    nan = np.isnan(a).any(-1)
    safe = np.where(np.isnan(a), -np.inf, a)
    rec[..., 4] = safe.max(-1)
    rec[..., 5] = safe.argmax(-1)              # the first maximum
    rec[nan, :5] = np.nan                      # a NaN row: NaN in the five value columns, whatever its segments hold ...
    rec[nan, 5] = -1                           # ... and no peak
    return rec


def slots(parent_ids, lengths):
    """-> (slot [B,S,W], Lb [B]): the slot hypothesis w passes through at column t < Lb = min(S, max_w lengths) (gather_tree's chain)."""
    par = np.asarray(parent_ids).astype(np.int64)
    S, nB, W = par.shape
    slot = np.zeros((nB, S, W), np.int64)
    Lb = np.minimum(S, np.asarray(lengths).reshape(nB, W).max(axis=1)).astype(int)
    for b in range(nB):
        for w in range(W):
            p = w
            for t in range(Lb[b] - 1, -1, -1):
                p = min(max(p, 0), W - 1)
                slot[b, t, w] = p
                p = par[t, b, p]
    return slot, Lb


def _quot(m1, m0, dtype):
    m1, m0 = np.asarray(m1, dtype), np.asarray(m0, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(m0 == 0, dtype(-1), m1 / np.where(m0 == 0, dtype(1), m0)).astype(dtype)


def finalize(step_moves, parent_ids, lengths, dtype=np.float64):
    """dtype float32: numpy's correctly rounded fp32 division of fp32 records -- what k_dec_finalize_moves computes, bit for bit."""
    rec = np.asarray(step_moves, dtype)
    par = np.asarray(parent_ids).astype(np.int64)
    S, nB, W = par.shape
    ln = np.asarray(lengths).reshape(nB, W).astype(int)
    slot, _ = slots(par, ln)
    out = dict(raw_pos=np.full((nB, S, W), -1, dtype), raw_mass=np.zeros((nB, S, W), dtype), event_pos=np.full((nB, S, W), -1, dtype),
               event_mass=np.zeros((nB, S, W), dtype), peak=np.full((nB, S, W), -1, np.int32), peak_weight=np.zeros((nB, S, W), dtype))
    for b in range(nB):
        for w in range(W):
            for t in range(min(S, ln[b, w])):
                r = rec[t, b, min(max(par[t, b, slot[b, t, w]], 0), W - 1)]
                out["raw_mass"][b, t, w], out["event_mass"][b, t, w], out["peak_weight"][b, t, w] = r[0], r[2], r[4]
                out["raw_pos"][b, t, w] = _quot(r[1], r[0], dtype)
                out["event_pos"][b, t, w] = _quot(r[3], r[2], dtype)
                out["peak"][b, t, w] = int(r[5])
    return out


def tfa_lengths(step_ids, parent_ids, end_token):
    ids, par = np.asarray(step_ids).astype(np.int64), np.asarray(parent_ids).astype(np.int64)
    S, nB, W = ids.shape
    fin, ln = np.zeros((nB, W), bool), np.zeros((nB, W), np.int64)
    for s in range(S):                       # TFA: len' = len[parent] + !fin[parent], fin' = fin[parent] | id == end
        pf, pl = np.take_along_axis(fin, par[s], 1), np.take_along_axis(ln, par[s], 1)
        ln, fin = pl + (~pf).astype(np.int64), pf | (ids[s] == end_token)
    return ln


def moves_reference(step_alignments, step_ids, parent_ids, lengths, T_r, end_token):
    """step_alignments [S,B,W,T_m], step_ids / parent_ids [S,B,W] of a whole-slab decode (every chunk holds all S steps), lengths
    [B,W], the split index T_r (T_m in raw mode, 0 in event mode) -> dict of the six outputs [B,S,W] in fp64 (peak int32)."""
    ln = np.asarray(lengths).reshape(np.asarray(parent_ids).shape[1:])
    assert (tfa_lengths(step_ids, parent_ids, end_token) == ln).all(), "lengths are not those of these records"
    return finalize(records(step_alignments, T_r), parent_ids, ln)
