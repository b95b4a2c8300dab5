"""Every configuration the C-ABI accepts, held to the fp64 oracle (1e-4, and the twin-relative bound of test_parity_gpu._assert_twin).

rv_create takes a vocabulary of 2..8 tokens, any start / end / pad id inside it, any input padding value, 1..8 encoder layers, 1..4
decoder cells and a widest beam of 1..8; the other GPU modules run 7 tokens, ids 2 / 1 / 0, padding 0.0 and depths 1-3.  Here the
decode families of test_kernel_forms_gpu run under five other configurations (CONFIGS), encoders of depth 4 and 8 run every
recurrence form, the C entry points are called with sentinel-filled buffers so that the columns beyond the slab's last step are
seen, and what rv_create and the calls refuse is checked by message.

A configuration reaches the library through the public constructor: a tokenizer of the duck type of data_loader.NucTokenizer
(_Tokenizer) gives the vocabulary and the three ids, input_padding_value the padding value.

Seeds.  A case only bites when its chunks finish at different steps and its beams emit every token, and it only compares whole
calls when the fp32 decode stays on the fp64 one.  For each (configuration, family) the weight seed was searched on the CPU, from
70 + V upwards, with the oracle's numpy fp32 twin standing in for the GPU: the first seed (at end-token bias 0.05; for E with
eight encoder layers, where twelve seeds at 0.05 / 0.3 / -0.3 / 0.6 and eighteen at 0.1 / 0.08 / 0.12 gave none, at 0.0) at which EVERY beam call of the family has chunks finishing at two or more different steps, one of them before step L - 1,
all V ids in its step_ids, and at most one of the six chunks leaving the fp64 decode.  SEEDS holds what that search found; the test
asserts the conditions again, on the fp64 decode (_well_chosen) and on the device's result (at most one chunk excused)."""
import ctypes

import numpy as np
import pytest

from test_parity_gpu import _assert_twin, _emitting_flat, _memory_errors, _twin_beam, _twin_greedy
from test_kernel_forms_gpu import (ATTEND, B, FLASH, FORM_TOL, PERSIST, REC, REC_MX, REC_PROJ, TOL, _beam, _check_beam,
                                   _check_forms_agree, _check_greedy, _f, _handle, _rows, _set, _slab, ENCODER)

pytestmark = pytest.mark.gpu

TR, TE, L = 70, 12, 16
TM = TR + TE                                          # k_dec_persist NIT 8, k_dec_attend TB 7; B <= 320: attend_threads 512
SENTINEL = 0x7F7F7F7F                                 # a large int32, and a finite float32 (3.39e38)

# name -> (vocab, start, end, pad, input padding value)
CONFIGS = {
    "A": (8, 7, 0, 3, -1.0),      # W * V = 64 candidates at beam 8; end token 0; pad token non-zero; negative padding
    "B": (2, 0, 1, 0, 0.0),       # V < W: step 0 has fewer finite candidates than beams; start == pad
    "C": (5, 4, 2, 0, 2.5),       # odd V; a padding value of ordinary sample magnitude
    "D": (3, 1, 0, 2, 0.0),       # V < 4: the first float4 of a beam's logits only partly valid
    "E": (8, 0, 7, 7, 0.0),       # start token 0; pad == end == last id
}


class _Tokenizer:
    """data_loader.NucTokenizer's duck type over another vocabulary: '' / '^' / '$' at the pad / end / start id (ids may coincide),
    letters at every other id."""

    def __init__(self, vocab, start, end, pad):
        self.word_index = {"": pad, "^": end, "$": start}
        letters = iter("acgtmnh")
        for i in range(vocab):
            if i not in (start, end, pad):
                self.word_index[next(letters)] = i
        self.index_word = {i: w for w, i in self.word_index.items()}
        assert len(self.index_word) == vocab


def _tokenizer(name):
    return _Tokenizer(*CONFIGS[name][:4])


# family -> (attention, decoder cells, encoder layers, beams)
FAMILIES = {
    "luong1": ("luong", 1, 2, (8, 5)),
    "bahdanau1": ("bahdanau", 1, 2, (8,)),
    "luong2": ("luong", 2, 2, (5,)),
    "luong1_enc8": ("luong", 1, 8, (5,)),
    "luong4": ("luong", 4, 2, (8,)),
    "bahdanau4": ("bahdanau", 4, 2, (8,)),
}
FOUR_CELLS = ("A", "C")

# (configuration, family) -> (weight seed, end-token bias): see "Seeds" above (the slab's seed is 1000 + the weight seed)
SEEDS = {
    ("A", "luong1"): (78, 0.05),
    ("A", "bahdanau1"): (78, 0.05),
    ("A", "luong2"): (78, 0.05),
    ("A", "luong1_enc8"): (81, 0.05),
    ("A", "luong4"): (78, 0.05),
    ("A", "bahdanau4"): (78, 0.05),
    ("B", "luong1"): (72, 0.05),
    ("B", "bahdanau1"): (72, 0.05),
    ("B", "luong2"): (72, 0.05),
    ("B", "luong1_enc8"): (72, 0.05),
    ("C", "luong1"): (75, 0.05),
    ("C", "bahdanau1"): (75, 0.05),
    ("C", "luong2"): (75, 0.05),
    ("C", "luong1_enc8"): (75, 0.05),
    ("C", "luong4"): (75, 0.05),
    ("C", "bahdanau4"): (75, 0.05),
    ("D", "luong1"): (73, 0.05),
    ("D", "bahdanau1"): (73, 0.05),
    ("D", "luong2"): (73, 0.05),
    ("D", "luong1_enc8"): (73, 0.05),
    ("E", "luong1"): (78, 0.05),
    ("E", "bahdanau1"): (78, 0.05),
    ("E", "luong2"): (78, 0.05),
    ("E", "luong1_enc8"): (80, 0.0),
}

PERSIST_ON = dict(persistent_decode=1, debug_taps=0, persist_taps=1, use_graph=1, flash_attend=1)
PER_STEP = dict(persistent_decode=0, debug_taps=1, persist_taps=0)


def _finish_steps(taps):
    """The step at which each chunk's last beam finished in the fp64 decode (S when it never did)."""
    return np.minimum(taps["lengths"].max(axis=1), taps["step_ids"].shape[0]).astype(int)


def _well_chosen(taps, V, tag):
    """The conditions on a case's inputs, on the oracle's side: finishing steps differ, one chunk finishes early, every id is used."""
    fin = _finish_steps(taps)
    assert len(set(fin.tolist())) >= 2 and fin.min() < L - 1, (tag, "badly chosen: the chunks finish at", fin.tolist())
    used = set(np.unique(taps["step_ids"]).tolist())
    assert used == set(range(V)), (tag, "badly chosen: ids in use", sorted(used))
    return fin


def _runs(att, D, W):
    """(label, options, the decode form they must run, persistent?) for one (family, beam)."""
    nit, tb = 8, 7
    if D == 4:
        want = _f(ATTEND, W, tb)
        return [(f"per-step graph {g}", dict(PER_STEP, use_graph=g, flash_attend=1), want, False) for g in (0, 1)]
    if D == 2:
        return [(f"ATT {a}", dict(PERSIST_ON, matrix_attention=1, matrix_cell=c), _f(PERSIST, W, nit, 2, a), True) for a, c in ((3, 1), (0, 0))]
    if att == "bahdanau":
        runs = [(f"ATT {a}", dict(PERSIST_ON, matrix_attention=1, matrix_cell=c), _f(PERSIST, W, nit, 1, a), True) for a, c in ((4, 1), (1, 0))]
        return runs + [(f"per-step graph {g}", dict(PER_STEP, use_graph=g, flash_attend=1), _f(ATTEND, W, tb), False) for g in (0, 1)]
    runs = [(f"ATT {a}", dict(PERSIST_ON, matrix_attention=m, matrix_cell=c), _f(PERSIST, W, nit, 1, a), True)
            for a, m, c in ((3, 1, 1), (2, 1, 0), (0, 0, 0))]
    for g in (0, 1):
        if W <= 5:
            runs.append((f"single-pass graph {g}", dict(PER_STEP, use_graph=g, flash_attend=1), _f(FLASH, W, 512), False))
            runs.append((f"two-pass graph {g}", dict(PER_STEP, use_graph=g, flash_attend=0), _f(ATTEND, W, tb), False))
        else:
            runs.append((f"two-pass graph {g}", dict(PER_STEP, use_graph=g, flash_attend=1), _f(ATTEND, W, tb), False))
    return runs


def _worst(r, o, n):
    """max |logits - fp64| and max |alignments - fp64| over the steps each chunk agrees with the fp64 decode."""
    lg = max((float(np.abs(r["lg"][:k, b] - o["step_logits"][:k, b]).max()) for b, k in enumerate(n) if k), default=0.0)
    al = max((float(np.abs(r["al"][:k, b] - o["step_alignments"][:k, b]).max()) for b, k in enumerate(n) if k), default=0.0)
    return lg, al


CASES = [(c, f) for c in CONFIGS for f in FAMILIES if f[-1] != "4" or c in FOUR_CELLS]


@pytest.mark.parametrize("name,fam", CASES, ids=[f"{c}-{f}" for c, f in CASES])
def test_configuration_against_fp64(rv, oracle, name, fam):
    """One decode family under one configuration, one slab (the mask patterns of test_kernel_forms_gpu._slab with the configuration's
    padding value): every form of the family -- persistent ATT forms, the per-step kernels with use_graph 0 and 1, greedy search --
    against ONE fp64 oracle pass per beam, by _check_beam / _check_greedy, the form asserted through kernel_forms, the persistent
    forms against each other; at most one of the six chunks may leave the fp64 decode at a near-tie."""
    V, start, end, pad_token, pad = CONFIGS[name]
    attention, D, enc_depth, beams = FAMILIES[fam]
    seed, bias = SEEDS[name, fam]
    bc, w = _handle(rv, "joint", attention, D, seed, Tr_max=TR, Te_max=TE, L=L, tokenizer=_tokenizer(name), pad=pad,
                    enc_depth=enc_depth, end_bias=bias)
    cfg = bc.cfg.oracle_cfg()
    assert (bc.cfg.vocab, cfg["start_token"], cfg["end_token"], bc.cfg.pad_token, cfg["padding_value"]) == (V, start, end, pad_token, pad)
    raw, ev = _slab("joint", TR, TE, seed=1000 + seed, pad=pad)
    for W in beams:
        taps = {}
        otok, osc = oracle.beam_search(w, cfg, raw, ev, W, L, dtype=np.float64, taps=taps)
        fin = _well_chosen(taps, V, f"{name} {fam} W={W}")
        twin = _twin_beam(oracle, w, cfg, raw, ev, W, L, taps, osc, f"config {name} {fam} W={W}")
        got, worst_lg, worst_al, ran = {}, 0.0, 0.0, []
        for label, opts, want, persist in _runs(attention, D, W):
            tag = f"config {name} {fam} W={W} {label}"
            _set(bc, opts)
            r = _beam(bc, (raw, ev), W, L, TM, persist=persist, V=V)
            assert r["forms"] == {want}, (tag, sorted(r["forms"]))
            n, left = _check_beam(oracle, r, taps, otok, osc, W, end, tag, twin)
            assert len(left) <= 1, (tag, "badly chosen: chunks that left the fp64 decode", sorted(left))
            lg, al = _worst(r, taps, n)
            worst_lg, worst_al = max(worst_lg, lg), max(worst_al, al)
            ran.append(f"{label} {want[:5]}" + (f" (chunk {sorted(left)} left at a near-tie)" if left else ""))
            if persist:
                got[label] = (r, n, left)
        ref = next(iter(got), None)
        for label in got:
            if label != ref:
                _check_forms_agree(got[ref], got[label], f"{name} {fam} W={W} {ref} vs {label}")
        print(f"config {name} {CONFIGS[name]} {fam} W={W} seed {seed} bias {bias}: finish steps {fin.tolist()}; "
              f"worst |logits - fp64| {worst_lg:.2e}, |alpha - fp64| {worst_al:.2e}; ran: " + "; ".join(ran))
    if fam == "luong1":
        gtaps = {}
        og, olg = oracle.greedy_search(w, cfg, raw, ev, L, dtype=np.float64, taps=gtaps)
        ends = [int(np.argmax(row == end)) if (row == end).any() else og.shape[1] for row in og]
        assert len(set(ends)) >= 2, (name, "badly chosen: greedy chunks end at", ends)
        gtwin = _twin_greedy(oracle, w, cfg, raw, ev, L, og, olg, gtaps, f"config {name} greedy")
        for a, m, c in ((3, 1, 1), (0, 0, 0)):
            _set(bc, dict(PERSIST_ON, matrix_attention=m, matrix_cell=c))
            forms = _check_greedy(bc, (raw, ev), L, TM, og, olg, gtaps, f"config {name} greedy ATT {a}", gtwin)
            assert forms == {_f(PERSIST, 1, 8, 1, a)}, (name, a, sorted(forms))
        print(f"config {name} greedy: ATT 3 and 0, chunks end at {ends}")
    bc.close()


# ----------------------------------------------------------------------------------------------
# encoder depth 4 and 8
ENC_FORMS = [dict(wide_recurrence=1), dict(wide_recurrence=2), dict(wide_recurrence=0, fused_projection=1, split_projection=2),
             dict(wide_recurrence=0, fused_projection=0, split_projection=2), dict(wide_recurrence=0, fused_projection=1, split_projection=0),
             dict(wide_recurrence=0, fused_projection=1, split_projection=1)]


def _encoder_forms(mode, opts):
    """The recurrence forms a slab of 20 chunks runs (one chunk per workgroup in the packed-FMA kernels: no tail wave)."""
    feats = (1, 5) if mode == "joint" else (5,)
    if opts["wide_recurrence"] == 0:
        upper = _f(REC_PROJ, 1, opts["split_projection"]) if opts["fused_projection"] else _f(REC, 1, 0)
        return {_f(REC, 1, F) for F in feats} | {upper}
    ch = 16 if opts["wide_recurrence"] == 1 else 8
    return {_f(REC_MX, F, ch) for F in feats} | {_f(REC_MX, 0, ch)}


@pytest.mark.parametrize("mode", ["joint", "event"])
@pytest.mark.parametrize("enc_depth,name", [(4, "C"), (8, "A")])
def test_deep_encoders_against_fp64(rv, oracle, enc_depth, name, mode):
    """Four and eight encoder layers (the weight images of layers >= 1 are indexed by e * (enc_depth - 1) + l - 1), 20 chunks (two
    workgroups of the 16-chunk matrix form, three of the 8-chunk one, twenty of the packed-FMA kernels), padding in the configuration's
    own value: enc_output, keys and the per-step decode (debug_taps) against fp64 for every recurrence form, the forms asserted
    through kernel_forms and compared with each other; the persistent decode on the default form."""
    V, start, end, pad_token, pad = CONFIGS[name]
    Bn, W = 20, 5
    Tr, Te = (TR, TE) if mode == "joint" else (0, 40)
    Tm = Tr + Te
    bc, w = _handle(rv, mode, "luong", 1, seed=50 + enc_depth, Tr_max=max(Tr, 1), Te_max=max(Te, 1), L=L, max_batch=Bn,
                    tokenizer=_tokenizer(name), pad=pad, enc_depth=enc_depth)
    cfg = bc.cfg.oracle_cfg()
    rng = np.random.default_rng(enc_depth)
    raw = rng.standard_normal((Bn, Tr, 1)).astype(np.float32)
    ev = rng.standard_normal((Bn, Te, 5)).astype(np.float32)
    for b in range(3, Bn, 5):                         # interior padding, one feature of an event; a suffix; all but the last step
        if Tr:
            raw[b, [31, 32, 63, 64, Tr - 1]] = pad
        ev[b, rng.integers(0, Te), b % 5] = pad
    ev[1, Te - Te // 3:] = pad
    ev[17, :-1] = pad
    if Tr:
        raw[1, Tr - Tr // 3:] = pad
        raw[17] = pad
    x = (raw, ev) if mode == "joint" else ev
    r_, e_ = (raw, ev) if mode == "joint" else (None, ev)
    taps = {}
    otok, osc = oracle.beam_search(w, cfg, r_, e_, W, L, dtype=np.float64, taps=taps)
    twins = _twin_beam(oracle, w, cfg, r_, e_, W, L, taps, osc, f"enc_depth {enc_depth} {mode} config {name}")
    twin = twins["enc_output"]
    ref = None
    for opts in ENC_FORMS:
        tag = f"enc_depth {enc_depth} {mode} config {name} {opts}"
        _set(bc, dict(PER_STEP, use_graph=1, flash_attend=0, **opts))
        r = _beam(bc, x, W, L, Tm, persist=False, V=V, B=Bn)
        forms = {f for f in _rows(bc, "kernel_forms") if f[0] in ENCODER}
        assert forms == _encoder_forms(mode, opts), (tag, sorted(forms))
        enc = bc.get_tensor("enc_output").reshape(Bn, Tm, 256)
        keys = bc.get_tensor("keys").reshape(Bn, Tm, 128)
        e_enc, e_keys = float(np.abs(enc - taps["enc_output"]).max()), float(np.abs(keys - taps["keys"]).max())
        n, left = _check_beam(oracle, r, taps, otok, osc, W, end, tag, twins, B=Bn)
        lg = max((float(np.abs(r["lg"][:k, b] - taps["step_logits"][:k, b]).max()) for b, k in enumerate(n) if k), default=0.0)
        print(f"{tag}: |enc_output - fp64| {e_enc:.2e} (numpy fp32 twin {twin:.2e}), |keys - fp64| {e_keys:.2e}, |logits - fp64| {lg:.2e}, "
              f"chunks that left at a near-tie {sorted(left)}; forms {sorted(f[:3] for f in forms)}")
        assert e_enc < TOL, (tag, "enc_output vs fp64", e_enc)
        assert e_keys < TOL, (tag, "keys vs fp64", e_keys)
        _assert_twin(_memory_errors(enc, keys, taps), twins, tag)
        if ref is None:
            ref = enc
        else:
            assert np.abs(enc - ref).max() < FORM_TOL, (tag, "enc_output between forms", float(np.abs(enc - ref).max()))
    _set(bc, dict(PERSIST_ON, matrix_attention=1, matrix_cell=1, wide_recurrence=1, fused_projection=1, split_projection=2))
    r = _beam(bc, x, W, L, Tm, persist=True, V=V, B=Bn)
    assert r["forms"] == {_f(PERSIST, W, min(k for k in (2, 8, 11) if Tm <= 32 * k), 1, 3)}, sorted(r["forms"])
    _check_beam(oracle, r, taps, otok, osc, W, end, f"enc_depth {enc_depth} {mode} persistent", twins, B=Bn)
    bc.close()


# ----------------------------------------------------------------------------------------------
# the output contract beyond step S, through the C entry points
def _filled(shape, dtype):
    """An output buffer no byte of which the call may leave as it was."""
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x7F, np.uint8).view(dtype).reshape(shape)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _no_sentinel(*arrays):
    for a in arrays:
        a = np.ascontiguousarray(a)
        assert (a.view(np.uint8).reshape(-1, a.dtype.itemsize) != 0x7F).any(axis=1).all(), "an element the call did not write"


def _beam_entry_points(bc, raw, ev, W, L=L):
    """(name, tokens [B, L-1], scores [B, L-1], S) of every beam-search entry point on sentinel-filled buffers."""
    import torch
    lib, h, S = bc._lib, bc._h, ctypes.c_int32(-1)
    Bn, steps = raw.shape[0], L - 1
    dims = (Bn, raw.shape[1], ev.shape[1], W, L)
    host = lambda: (_filled((Bn, steps), np.int32), _filled((Bn, steps), np.float32))
    dev = lambda: (torch.full((Bn, steps), SENTINEL, dtype=torch.int32, device=bc.device),
                   torch.full((Bn, steps), SENTINEL, dtype=torch.int32, device=bc.device).view(torch.float32))
    d_raw, d_ev = torch.from_numpy(raw).to(bc.device), torch.from_numpy(ev).to(bc.device)
    dp = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize(bc.device)
    out = []
    tk, sc = host()
    bc._check(lib.rv_beam_search(h, _p(raw), _p(ev), *dims, _p(tk), _p(sc), ctypes.byref(S)), "rv_beam_search")
    out.append(("rv_beam_search", tk, sc, S.value))
    dt, ds = dev()
    torch.cuda.synchronize(bc.device)
    bc._check(lib.rv_beam_search_dev(h, dp(d_raw), dp(d_ev), *dims, dp(dt), dp(ds), ctypes.byref(S)), "rv_beam_search_dev")
    out.append(("rv_beam_search_dev", dt.cpu().numpy(), ds.cpu().numpy(), S.value))
    t = ctypes.c_int32(-1)
    tk, sc = host()
    bc._check(lib.rv_beam_search_submit(h, _p(raw), _p(ev), *dims, ctypes.byref(t)), "rv_beam_search_submit")
    bc._check(lib.rv_beam_search_collect(h, t.value, _p(tk), _p(sc), ctypes.byref(S)), "rv_beam_search_collect")
    out.append(("rv_beam_search_submit / _collect", tk, sc, S.value))
    dt, ds = dev()
    torch.cuda.synchronize(bc.device)
    bc._check(lib.rv_beam_search_submit_dev(h, dp(d_raw), dp(d_ev), *dims, dp(dt), dp(ds), ctypes.byref(t)), "rv_beam_search_submit_dev")
    bc._check(lib.rv_beam_search_collect_dev(h, t.value, ctypes.byref(S)), "rv_beam_search_collect_dev")
    out.append(("rv_beam_search_submit_dev / _collect_dev", dt.cpu().numpy(), ds.cpu().numpy(), S.value))
    return out


def _greedy_entry_points(bc, raw, ev, V, L=L):
    import torch
    lib, h, S = bc._lib, bc._h, ctypes.c_int32(-1)
    Bn, steps = raw.shape[0], L - 1
    dims = (Bn, raw.shape[1], ev.shape[1], L)
    tk, lg = _filled((Bn, steps), np.int32), _filled((Bn, steps, V), np.float32)
    bc._check(lib.rv_greedy_search(h, _p(raw), _p(ev), *dims, _p(tk), _p(lg), ctypes.byref(S)), "rv_greedy_search")
    out = [("rv_greedy_search", tk, lg, S.value)]
    d_raw, d_ev = torch.from_numpy(raw).to(bc.device), torch.from_numpy(ev).to(bc.device)
    dt = torch.full((Bn, steps), SENTINEL, dtype=torch.int32, device=bc.device)
    dl = torch.full((Bn, steps, V), SENTINEL, dtype=torch.int32, device=bc.device).view(torch.float32)
    dp = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize(bc.device)
    bc._check(lib.rv_greedy_search_dev(h, dp(d_raw), dp(d_ev), *dims, dp(dt), dp(dl), ctypes.byref(S)), "rv_greedy_search_dev")
    out.append(("rv_greedy_search_dev", dt.cpu().numpy(), dl.cpu().numpy(), S.value))
    return out


def _calls_entry_points(bc, raw, ev, W, L=L):
    lib, h, S, t = bc._lib, bc._h, ctypes.c_int32(-1), ctypes.c_int32(-1)
    Bn, steps = raw.shape[0], L - 1
    dims = (Bn, raw.shape[1], ev.shape[1], W, L)
    lut = bc._call_lut()
    bufs = lambda: (_filled((Bn, steps), np.uint8), _filled((Bn,), np.int32), _filled((Bn, steps), np.float32))
    bases, lens, probs = bufs()
    bc._check(lib.rv_beam_search_calls(h, _p(raw), _p(ev), *dims, _p(lut), _p(bases), _p(lens), _p(probs), ctypes.byref(S)), "rv_beam_search_calls")
    out = [("rv_beam_search_calls", bases, lens, probs, S.value)]
    bases, lens, probs = bufs()
    bc._check(lib.rv_beam_search_submit_calls(h, _p(raw), _p(ev), *dims, _p(lut), ctypes.byref(t)), "rv_beam_search_submit_calls")
    bc._check(lib.rv_beam_search_collect_calls(h, t.value, _p(bases), _p(lens), _p(probs), ctypes.byref(S)), "rv_beam_search_collect_calls")
    out.append(("rv_beam_search_submit_calls / _collect_calls", bases, lens, probs, S.value))
    return out


# configuration -> (weight seed, end-token bias, letter bias) of the weights that stop the slab early: the first seed from 70 + V, at
# end-token bias 1.3 with the letters at 1.0, at which the fp64 beam search (W 5) of the slab stops before step L - 1 with every
# chunk's best hypothesis ended before the slab's last step, the fp64 greedy search stops before L - 1 too, and the numpy fp32 twin
# returns the same tokens.  (Such weights end their best hypotheses at once; with random weights no seed of 36 tried per
# configuration both stopped early and called letters, so the letters come from a second set of weights: _emitting_flat at seed
# 70 + V, whose slab runs all L - 1 steps.)
CONTRACT_SEEDS = {"A": (80, 1.3, 1.0), "C": (75, 1.3, 1.0), "E": (78, 1.3, 1.0)}


@pytest.mark.parametrize("name", ["A", "C", "E"])
def test_outputs_beyond_the_last_step(rv, oracle, name):
    """include/ravvent_hip.h: tokens [B, L-1] hold pad_token and scores / greedy logits / probs 0 in the columns >= S, bases are
    zero-filled after a chunk's letters -- for every entry point, on the default path, the per-step kernels and the slab graph.
    basecaller.py never shows those columns (it returns [:, :S]); a C caller reads them.  Buffers come pre-filled with 0x7f bytes,
    one set of weights makes the slab stop early (S < L - 1), and pad tokens 3 / 7 (A / E) tell a pad fill from a zero fill.  Inside
    [0, S) a chunk's columns after its own end hold end_token (0 in A, 7 in E).  A second set of weights calls letters: the fused
    post-processing follows the tokenizer (strings, lengths, zero-filled bases, probs)."""
    V, start, end, pad_token, pad = CONFIGS[name]
    seed, bias, letter_bias = CONTRACT_SEEDS[name]
    W = 5
    tk_ = _tokenizer(name)
    bc, _ = _handle(rv, "joint", "luong", 1, seed, Tr_max=TR, Te_max=TE, L=L, tokenizer=tk_, pad=pad)
    cfg = bc.cfg.oracle_cfg()
    stop = rv.weights.init_weights(bc.cfg, seed=seed, gain=1.5)
    stop["b_fc"][[t for t in range(V) if t not in (start, end, pad_token)]] = letter_bias
    stop["b_fc"][end] = bias
    for kind, flat, slab_seed in (("stop", stop, 1000 + seed), ("emit", _emitting_flat(rv, bc.cfg, seed=70 + V), 1070 + V)):
        bc.set_weights_flat(flat)
        w = rv.weights.flat_to_nested(bc.cfg, flat)
        raw, ev = _slab("joint", TR, TE, seed=slab_seed, pad=pad)
        otok, osc = oracle.beam_search(w, cfg, raw, ev, W, L, dtype=np.float64)
        og, olg = oracle.greedy_search(w, cfg, raw, ev, L, dtype=np.float64)
        So, Sg = otok.shape[1], og.shape[1]
        own_end = [int(np.argmax(row == end)) if (row == end).any() else So for row in otok]
        strings = oracle.tokens_to_nuc_sequences(otok, tk_.index_word)
        if kind == "stop":
            assert So < L - 1 and Sg < L - 1, (name, "badly chosen: steps", So, Sg)
            assert max(own_end) + 1 < So, (name, "badly chosen: chunks end at", own_end)
        else:
            assert len(set("".join(strings))) >= 2, (name, "badly chosen: calls", strings)
        assert bc.tokens_to_nuc_sequences(otok) == strings
        _contract(bc, oracle, name, kind, raw, ev, W, V, end, pad_token, otok, osc, og, olg, own_end, strings)
        print(f"config {name} {kind}: S = {So} (greedy {Sg}) of {L - 1}, chunks end at {own_end}, calls {strings}")
    bc.close()


def _contract(bc, oracle, name, kind, raw, ev, W, V, end, pad_token, otok, osc, og, olg, own_end, strings):
    So, Sg = otok.shape[1], og.shape[1]
    for mode_opts in (dict(persistent_decode=1, slab_graph=0), dict(persistent_decode=0, slab_graph=0), dict(persistent_decode=1, slab_graph=1)):
        _set(bc, mode_opts)
        ref = None
        for entry, tok, sc, S in _beam_entry_points(bc, raw, ev, W):
            tag = f"config {name} {kind} {mode_opts} {entry}"
            assert S == So, (tag, S, So)
            assert (tok[:, :S] == otok).all(), (tag, "tokens")
            assert np.abs(sc[:, :S] - osc).max() < TOL, (tag, "scores")
            for b in range(B):
                assert (tok[b, own_end[b]:S] == end).all(), (tag, b, "columns after the chunk's own end")
            assert (tok[:, S:] == pad_token).all(), (tag, "tokens beyond S", tok[:, S:].tolist())
            assert (sc[:, S:].view(np.uint32) == 0).all(), (tag, "scores beyond S")
            _no_sentinel(tok, sc)
            if ref is None:
                ref = (tok, sc)
            else:
                assert np.array_equal(tok, ref[0]) and np.array_equal(sc.view(np.uint32), ref[1].view(np.uint32)), (tag, "differs from rv_beam_search")
        for entry, tok, lg, S in _greedy_entry_points(bc, raw, ev, V):
            tag = f"config {name} {kind} {mode_opts} {entry}"
            assert S == Sg, (tag, S, Sg)
            assert (tok[:, :S] == og).all(), (tag, "tokens")
            assert np.abs(lg[:, :S] - olg).max() < TOL, (tag, "logits")
            assert (tok[:, S:] == pad_token).all(), (tag, "tokens beyond S", tok[:, S:].tolist())
            assert (lg[:, S:].view(np.uint32) == 0).all(), (tag, "logits beyond S")
            _no_sentinel(tok, lg)
        host_probs = oracle.calc_prob_logits_beam_search_scores(ref[1][:, :So])
        for entry, bases, lens, probs, S in _calls_entry_points(bc, raw, ev, W):
            tag = f"config {name} {kind} {mode_opts} {entry}"
            assert S == So, (tag, S, So)
            assert lens.tolist() == [len(s) for s in strings], (tag, lens.tolist(), strings)
            for b in range(B):
                assert bases[b, :lens[b]].tobytes().decode("ascii") == strings[b], (tag, b)
                assert (bases[b, lens[b]:] == 0).all(), (tag, b, "bases beyond the chunk's letters")
            assert np.abs(probs[:, :S] - host_probs).max() < 1e-6, (tag, "probs")
            assert (probs[:, S:].view(np.uint32) == 0).all(), (tag, "probs beyond S")
            _no_sentinel(lens, probs)


# ----------------------------------------------------------------------------------------------
# what rv_create and the calls refuse
REFUSED = [
    (dict(vocab=1), "RV_EINVAL", r"vocab 1 outside \[2,8\]"),
    (dict(vocab=9), "RV_EINVAL", r"vocab 9 outside \[2,8\]"),
    (dict(start_token=7), "RV_EINVAL", "token id 7 outside vocab"),
    (dict(end_token=7), "RV_EINVAL", "token id 7 outside vocab"),
    (dict(pad_token=-1), "RV_EINVAL", "token id -1 outside vocab"),
    (dict(enc_depth=0), "RV_EINVAL", r"encoder_depth 0 outside \[1,8\]"),
    (dict(enc_depth=9), "RV_EINVAL", r"encoder_depth 9 outside \[1,8\]"),
    (dict(dec_depth=0), "RV_EUNSUPPORTED", r"decoder_depth 0 outside \[1,4\]"),
    (dict(dec_depth=5), "RV_EUNSUPPORTED", r"decoder_depth 5 outside \[1,4\]"),
    (dict(enc_units=64), "RV_EUNSUPPORTED", r"enc_units = dec_units = 128 \(got 64, 128\)"),
    (dict(dec_units=256), "RV_EUNSUPPORTED", r"enc_units = dec_units = 128 \(got 128, 256\)"),
    (dict(max_beam=0), "RV_EINVAL", r"max_beam 0 outside \[1,8\]"),
    (dict(max_beam=9), "RV_EINVAL", r"max_beam 9 outside \[1,8\]"),
]


@pytest.mark.parametrize("fields,code,message", REFUSED, ids=[f"{k}={v}" for f, _, _ in REFUSED for k, v in f.items()])
def test_rv_create_refuses(rv, fields, code, message):
    """Each limit of include/ravvent_hip.h's RvConfig, one step outside: no handle, the code and the message."""
    import re
    lib = rv._capi.load_library()
    cfg = rv.config.RvConfig(max_batch=4, **fields)
    h = ctypes.c_void_p()
    ccfg = cfg.to_c()
    rc = lib.rv_create(ctypes.byref(ccfg), ctypes.byref(h))
    assert rv._capi.ERROR_NAMES.get(rc) == code and not h, (fields, rc)
    assert re.search(message, lib.rv_last_error(None).decode()), (fields, lib.rv_last_error(None))
    with pytest.raises(rv._capi.RavventHipError, match=message):
        rv._capi.check(lib, None, rc, "rv_create")


def test_max_beam_bounds_the_calls(rv, oracle):
    """A handle created for beams up to 3 runs W = 3 (against fp64) and refuses W = 4, in every beam entry point."""
    name = "D"
    V, start, end, pad_token, pad = CONFIGS[name]
    seed, bias = SEEDS[name, "luong1"]
    bc = rv.Basecaller(128, 128, 128, _tokenizer(name), "joint", pad, max_batch=B, max_raw_len=TR, max_event_len=TE, max_output_len=L,
                       max_beam=3)
    assert bc.cfg.max_beam == 3
    flat = rv.weights.init_weights(bc.cfg, seed=seed, gain=1.5)
    flat["b_fc"][end] = bias
    bc.set_weights_flat(flat)
    w, cfg = rv.weights.flat_to_nested(bc.cfg, flat), bc.cfg.oracle_cfg()
    raw, ev = _slab("joint", TR, TE, seed=1000 + seed, pad=pad)
    taps = {}
    otok, osc = oracle.beam_search(w, cfg, raw, ev, 3, L, dtype=np.float64, taps=taps)
    bc.set_option("persist_taps", 1)
    r = _beam(bc, (raw, ev), 3, L, TM, persist=True, V=V)
    assert r["forms"] == {_f(PERSIST, 3, 8, 1, 3)}, sorted(r["forms"])
    _check_beam(oracle, r, taps, otok, osc, 3, end, "max_beam 3, W 3", _twin_beam(oracle, w, cfg, raw, ev, 3, L, taps, osc, "max_beam 3, W 3"))
    for call in (lambda: bc.beam_search_prediction((raw, ev), 4, L), lambda: bc.submit_beam_search((raw, ev), 4, L),
                 lambda: bc.beam_search_calls((raw, ev), 4, L), lambda: bc.submit_calls((raw, ev), 4, L)):
        with pytest.raises(rv._capi.RavventHipError, match=r"beam width 4 outside \[1,3\]"):
            call()
    tok, _ = bc.beam_search_prediction((raw, ev), 3, L)              # the refusals left the handle usable
    assert (tok.numpy() == r["tok"]).all()
    bc.close()
