"""The cases of tests/test_gru_persist_gpu.py (the persistent GRU decode, option gru_persistent) and the numpy restatement of its folded
images, shared with tests/test_gru_persist.py, which proves on the reference alone that every case that is not already one of
tests/gru_cases.py is a fair probe.

The form list k_dec_persist_gru<W, NIT, ATT> is W = 1..8 x NIT in {2, 8, 11} x ATT in {3 Luong, 4 Bahdanau}.  NIT resident row groups
serve T_m <= 32 NIT, so one T_m per band: 57 = 50 + 7 (NIT 2), 230 = 200 + 30 (NIT 8), 352 (NIT 11: 100 + 252 joint for odd beam
widths, event-only 352 for even ones).  Every beam width in both attentions at every band: seventeen chunks with padded rows, one
encoder layer (the decode is what is probed), L = 12 at T_m 57, 8 at 230, 6 at 352.  From tests/gru_cases.py come the greedy
searches, tail-T1 (T_m = 2), the all-padding chunks and the two-layer long windows; FORMS says which form each case must launch.
Slab seeds: the first of 3, 4, 5, ... under which the fp32 twin stays on the fp64 decode on every chunk and the decode runs at least
two steps (tests/test_gru_persist.py asserts both; seed 3 does for all 48)."""
import functools

import numpy as np

import gru_cases as C
import gru_reference as G

BANDS = {2: (50, 7, 12), 8: (200, 30, 8), 11: (100, 252, 6)}      # NIT: (T_r, T_e, L)
ATT = {"luong": 3, "bahdanau": 4}
SEEDS = {}                                                          # (W, attention, NIT) -> slab seed where 3 does not do


def _new_case(W, att, nit):
    Tr, Te, L = BANDS[nit]
    mode = "joint"
    if nit == 11 and W % 2 == 0:
        mode, Tr, Te = "event", 0, 352
    return C._c(f"persist-W{W}-{att}-nit{nit}", 17, mode, Tr, Te, W=W, attention=att, L=L, slab_seed=SEEDS.get((W, att, nit), 3),
                pads=(15, 3) if nit == 2 else None)


NEW_CASES = [_new_case(W, att, nit) for W in range(1, 9) for att in ATT for nit in BANDS]
# cases of gru_cases.py that run through the persistent decode as they are (one decoder cell)
SHARED = ["search-greedy-luong", "search-greedy-bahdanau", "tail-T1", "allpad-greedy", "allpad-beam3", "long-joint-200+30",
          "long-joint-100+252", "lds-event-T352", "long-bahdanau-T352", "cell-N1-dec1-luong", "cell-N64-dec1-bahdanau"]
BY_NAME = {c.name: c for c in NEW_CASES}
BY_NAME.update({n: C.BY_NAME[n] for n in SHARED})
assert len(BY_NAME) == len(NEW_CASES) + len(SHARED)


def form(c):
    """(11, W, NIT, 1, ATT): the form the case must launch."""
    Tm = {"raw": c.Tr, "event": c.Te, "joint": c.Tr + c.Te}[c.mode]
    return (11, max(c.W, 1), min(n for n in BANDS if Tm <= 32 * n), 1, ATT[c.attention])


@functools.lru_cache(maxsize=None)
def fp64(rv, name):
    """gru_cases.fp64 for any case of BY_NAME."""
    if name in C.BY_NAME:
        return C.fp64(rv, name)
    c = BY_NAME[name]
    raw, ev = C.slab(rv, c)
    _, w = C.weights(rv, c.enc_depth, c.dec_depth, c.mode, c.attention)
    cfg = C.config(rv, c).oracle_cfg()
    taps = {}
    out = G.beam_search(w, cfg, raw, ev, c.W, c.L, taps=taps)
    return C._freeze(dict(raw=raw, ev=ev, w=w, cfg=cfg, out=tuple(C._freeze(a) for a in out), taps=taps))


@functools.lru_cache(maxsize=None)
def _twin(rv, name):
    """One fp32 pass of the reference over a new case: ({tensor: max |twin - fp64|}, the chunks on which it leaves the fp64 decode)."""
    from test_parity_gpu import _beam_errors, _memory_errors
    c, r = BY_NAME[name], fp64(rv, name)
    t = {}
    _, tsc = G.beam_search(r["w"], r["cfg"], r["raw"], r["ev"], c.W, c.L, dtype=np.float32, taps=t)
    S, nB = t["step_ids"].shape[:2]
    err, left = _beam_errors(t["step_logits"], t["step_alignments"], t["step_ids"], t["parent_ids"], np.full(nB, S), tsc, r["taps"], r["out"][1])
    err.update(_memory_errors(t["enc_output"], t["keys"], r["taps"]))
    return err, tuple(left)


def twin_errors(rv, name):
    """gru_cases.twin_errors for any case of BY_NAME."""
    return C.twin_errors(rv, name) if name in C.BY_NAME else _twin(rv, name)[0]


def twin_left(rv, name):
    """The chunks of a NEW case on which the fp32 twin leaves the fp64 decode (tests/test_gru_persist.py: none)."""
    return list(_twin(rv, name)[1])


# ---------------------------------------------------------------------------------------------- the folded images, restated in fp64
def fold_fp64(flat, V):
    """The tensors k_dec_persist_gru reads, from a bigru flat dict of one decoder cell, in fp64: the folded cell kernel K [256, 512]
    (rows ctx' then h; column tiles z, r, candidate-input, candidate-recurrent), the token table [V, 512], the bias [512], the
    output layer [256, V] on [ctx' | h] and the memory kernel [W_mem | A_c] [256, 256]."""
    u = 128
    W, U, b = (np.asarray(flat[f"dec_cells.0.{k}"], np.float64) for k in ("W", "U", "b"))
    Wt, Wa = W[:V], W[V:]
    A = np.asarray(flat["W_att"], np.float64)
    Ah, Ac = A[:u], A[u:]
    Wfc = np.asarray(flat["W_fc"], np.float64)
    z, r, h = slice(0, u), slice(u, 2 * u), slice(2 * u, 3 * u)
    K = np.zeros((2 * u, 4 * u))
    K[:u, :3 * u] = Wa
    K[u:, 0 * u:1 * u] = U[:, z] + Ah @ Wa[:, z]
    K[u:, 1 * u:2 * u] = U[:, r] + Ah @ Wa[:, r]
    K[u:, 2 * u:3 * u] = Ah @ Wa[:, h]
    K[u:, 3 * u:4 * u] = U[:, h]
    tok = np.zeros((V, 4 * u))
    tok[:, :3 * u] = Wt
    bias = np.concatenate([b[0, z] + b[1, z], b[0, r] + b[1, r], b[0, h], b[1, h]])
    out = np.concatenate([Wfc, Ah @ Wfc])
    mem = np.concatenate([np.asarray(flat["W_mem"], np.float64), Ac], axis=1)
    return dict(K=K, tok=tok, bias=bias, out=out, mem=mem)


def gates(z4, hp):
    """The gate phase of k_dec_persist_gru on the four tiles z4 [..., 512] and the parent's h."""
    u = hp.shape[-1]
    z = G._sigmoid(z4[..., :u])
    r = G._sigmoid(z4[..., u:2 * u])
    hh = np.tanh(z4[..., 2 * u:3 * u] + r * z4[..., 3 * u:])
    return z * hp + (1 - z) * hh
