"""Scoring given label sequences on the GPU: the forced decode (rv_teacher_forced*), the scoring kernel (rv_score_logits) and the
Basecaller methods in front of them, against the fp64 oracle.

Teacher forcing has no search: the GPU and the oracle are fed the same labels and cannot part ways, so EVERY step of EVERY chunk is
compared, in every case.  The fp64 reference is test_teacher_forced.forced_decode (the oracle's encode_input, setup_memory and
attention_step in a loop over target[:, s]); its numpy fp32 twin is the same loop with dtype=np.float32, and the GPU's logits are held
within 1e-4 of fp64 and within TWIN_K x the twin's error + TWIN_C (test_parity_gpu._assert_twin).  Loss and accuracy are held to
test_teacher_forced's numpy restatements of loss_function / masked_accuracy.

Shapes: B = 3 chunks, joint T_r = 27 + T_e = 6, so T_m = 33 crosses the 32-row edge of the persistent decode's row groups (NIT 2);
chunk 1's signal tail is padding.  L = 8 labels (7 steps), and L = 2 (one step) and L = 64 (the limit) once each.  Label rows: `$`,
bases, an early `^`, then padding; a row that starts with a base instead of `$`; a row that is all padding."""
import numpy as np
import pytest

from test_bench_config_gpu import TWIN_C, TWIN_K
from test_config_space_gpu import _tokenizer
from test_kernel_forms_gpu import ATTEND, FLASH, PERSIST, _decode_forms, _handle, _oracle_inputs, _rows, _set, _x
from test_parity_gpu import _assert_twin, _emitting_flat
from test_teacher_forced import (END, PAD, START, TRAIN_OMIT, VAL_OMIT, follow_labels, forced_decode, np_counts, np_loss, np_masked_accuracy,
                                 np_nll)

pytestmark = pytest.mark.gpu

TOL = 1e-4
B, TR, TE, L, V = 3, 27, 6, 8, 7


def _slab(nB=B, seed=1):
    """nB chunks of T_r = 27 samples and T_e = 6 events; chunk 1's tail is padding in both parts."""
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((nB, TR, 1)).astype(np.float32)
    ev = rng.standard_normal((nB, TE, 5)).astype(np.float32)
    if nB > 1:
        raw[1, TR - 9:] = 0.0
        ev[1, TE - 2:] = 0.0
    return raw, ev


def _labels(nB, L_, seed=7):
    """Rows of random bases behind `$`; row 0 ends early (`^`, then padding), row 1 starts with a base instead of `$`, row 2 is all
    padding; the pattern repeats every three rows with other letters."""
    rng = np.random.default_rng(seed)
    t = rng.integers(3, 7, size=(nB, L_)).astype(np.int32)
    t[:, 0] = START
    for b in range(nB):
        if b % 3 == 0 and L_ > 2:
            e = 1 + (L_ - 1) // 2
            t[b, e] = END
            t[b, e + 1:] = PAD
        elif b % 3 == 1:
            t[b, 0] = 3 + b % 4
        else:
            t[b] = PAD
    return t


# case -> (mode, attention, decoder cells, options, the decode form that must run)
PERSIST_ON = dict(persistent_decode=1)
CASES = {
    "joint": ("joint", "luong", 1, PERSIST_ON, (PERSIST, 1, 2, 1, 3)),
    "raw": ("raw", "luong", 1, PERSIST_ON, (PERSIST, 1, 2, 1, 3)),
    "event": ("event", "luong", 1, PERSIST_ON, (PERSIST, 1, 2, 1, 3)),
    "bahdanau": ("joint", "bahdanau", 1, PERSIST_ON, (PERSIST, 1, 2, 1, 4)),
    "two_cells": ("joint", "luong", 2, PERSIST_ON, (PERSIST, 1, 2, 2, 3)),
    "three_cells": ("joint", "luong", 3, PERSIST_ON, (FLASH, 1, 512, 0, 0)),            # no persistent form: the per-step kernels
    "bahdanau_two_cells": ("joint", "bahdanau", 2, PERSIST_ON, (ATTEND, 1, 2, 0, 0)),   # the same, two-pass attend
    "per_step": ("joint", "luong", 1, dict(persistent_decode=0), (FLASH, 1, 512, 0, 0)),
    "per_step_bahdanau": ("joint", "bahdanau", 1, dict(persistent_decode=0), (ATTEND, 1, 2, 0, 0)),
    "fma": ("joint", "luong", 1, dict(persistent_decode=1, matrix_attention=0, matrix_cell=0), (PERSIST, 1, 2, 1, 0)),
}


def _open(rv, case, seed=31, L_max=L, max_batch=B):
    mode, attention, D, opts, form = CASES[case]
    bc, w = _handle(rv, mode, attention, D, seed, Tr_max=TR, Te_max=TE, L=L_max, max_batch=max_batch)
    _set(bc, opts)
    return bc, w, mode, form


def _forced(bc, mode, raw, ev, target, device=False):
    """One forced call -> ForcedScores as numpy arrays."""
    x = _x(mode, raw, ev)
    if device:
        import torch
        x = tuple(torch.from_numpy(a).cuda() for a in x) if mode == "joint" else torch.from_numpy(x).cuda()
    r = bc._teacher_forced(x, target, TRAIN_OMIT)
    return type(r)(*[np.asarray(a.cpu()).copy() for a in r])


def _bound(gpu_lg, ref, twin_lg, tag):
    """The logits of one case on all L - 1 columns of all chunks: within 1e-4 of fp64 and within TWIN_K x the numpy fp32 twin's error +
    TWIN_C.  Returns the bound they met (the smaller of the two), from which the nll bound derives."""
    assert gpu_lg.shape == ref.shape and np.isfinite(gpu_lg).all(), (tag, gpu_lg.shape, ref.shape)
    err = {"logits": float(np.abs(gpu_lg - ref).max())}
    twin = {"logits": float(np.abs(twin_lg - ref).max())}
    _assert_twin(err, twin, tag)
    assert err["logits"] < TOL, (tag, err)
    return min(TOL, TWIN_K * twin["logits"] + TWIN_C)


def _check_scores(r, target, ref_lg, bound, tag):
    """nll within 2 x the logits' bound of the fp64 nll (log-softmax is 2-Lipschitz in the max norm: |lse(a) - lse(b)| <= |a - b|_max and
    |a_y - b_y| <= |a - b|_max), nll_sum the row's column-order fp32 sum of the returned nll, exact counts, sample_id the argmax."""
    real = target[:, 1:]
    assert np.array_equal(r.sample_id, np.argmax(r.logits, -1)), (tag, "sample_id is not the argmax of the returned logits")
    ref_nll = np_nll(ref_lg, real)
    d = float(np.abs(r.nll - ref_nll).max(initial=0.0))
    print(f"nll [{tag}]: max |gpu - fp64| {d:.2e}, bound {2 * bound:.2e}")
    assert d <= 2 * bound, (tag, "nll", d, 2 * bound)
    assert (r.nll[real == PAD] == 0).all(), (tag, "nll at a padding label")
    want = np.zeros(r.nll.shape[0], np.float32)
    for s in range(r.nll.shape[1]):
        want = want + r.nll[:, s]
    assert np.array_equal(r.nll_sum, want), (tag, "nll_sum is not the column-order sum")
    assert np.array_equal(r.n_labels, (real != PAD).sum(-1)), (tag, "n_labels")
    n_match, n_counted = np_counts(real, r.sample_id, TRAIN_OMIT)
    assert np.array_equal(r.n_match, n_match) and np.array_equal(r.n_counted, n_counted), (tag, "accuracy counts")


@pytest.fixture(scope="module")
def main_case(rv, oracle):
    """The main case's handle, slab, labels and both reference passes, shared by the tests that need them (none changes them)."""
    bc, w, mode, form = _open(rv, "joint", max_batch=17)
    raw, ev = _slab()
    target = _labels(B, L)
    cfg = bc.cfg.oracle_cfg()
    ref, ref_ids = forced_decode(oracle, w, cfg, raw, ev, target)
    twin, _ = forced_decode(oracle, w, cfg, raw, ev, target, dtype=np.float32)
    yield dict(bc=bc, w=w, raw=raw, ev=ev, target=target, ref=ref, ref_ids=ref_ids, twin=twin, form=form)
    bc.close()


# ---------------------------------------------------------------------------------------------- 1, 4, 6: logits, sample_id, nll
@pytest.mark.parametrize("case", list(CASES))
def test_forced_logits_against_fp64(rv, oracle, case):
    bc, w, mode, form = _open(rv, case)
    raw, ev = _slab()
    target = _labels(B, L)
    cfg = bc.cfg.oracle_cfg()
    oraw, oev = _oracle_inputs(mode, raw, ev)
    ref, _ = forced_decode(oracle, w, cfg, oraw, oev, target)
    twin, _ = forced_decode(oracle, w, cfg, oraw, oev, target, dtype=np.float32)
    r = _forced(bc, mode, raw, ev, target)
    assert _decode_forms(bc) == {form}, (case, "the intended kernel did not run", _decode_forms(bc))
    bound = _bound(r.logits, ref, twin, case)
    _check_scores(r, target, ref, bound, case)
    bc.close()


@pytest.mark.parametrize("case", ["joint", "per_step"])
def test_a_single_step(rv, oracle, case):
    bc, w, mode, form = _open(rv, case)
    raw, ev = _slab()
    target = _labels(B, 2)
    ref, _ = forced_decode(oracle, w, bc.cfg.oracle_cfg(), raw, ev, target)
    twin, _ = forced_decode(oracle, w, bc.cfg.oracle_cfg(), raw, ev, target, dtype=np.float32)
    r = _forced(bc, mode, raw, ev, target)
    assert r.logits.shape == (B, 1, V) and _decode_forms(bc) == {form}
    _check_scores(r, target, ref, _bound(r.logits, ref, twin, case + " L=2"), case + " L=2")
    bc.close()


def test_the_longest_label_row(rv, oracle):
    bc, w, mode, form = _open(rv, "joint", L_max=64)
    raw, ev = _slab()
    target = _labels(B, 64)
    ref, _ = forced_decode(oracle, w, bc.cfg.oracle_cfg(), raw, ev, target)
    twin, _ = forced_decode(oracle, w, bc.cfg.oracle_cfg(), raw, ev, target, dtype=np.float32)
    r = _forced(bc, mode, raw, ev, target)
    assert r.logits.shape == (B, 63, V) and _decode_forms(bc) == {form}
    _check_scores(r, target, ref, _bound(r.logits, ref, twin, "L=64"), "L=64")
    bc.close()


def test_host_and_device_calls_agree(main_case):
    m = main_case
    host = _forced(m["bc"], "joint", m["raw"], m["ev"], m["target"])
    dev = _forced(m["bc"], "joint", m["raw"], m["ev"], m["target"], device=True)
    for a, b_, name in zip(host, dev, host._fields):
        assert a.tobytes() == b_.tobytes(), name


# ---------------------------------------------------------------------------------------------- 2: self-consistency, bit for bit
@pytest.mark.parametrize("case", ["joint", "bahdanau", "per_step", "per_step_bahdanau"])
def test_forced_with_the_greedy_ids_is_the_greedy_search(rv, case):
    """target = [start | the greedy search's sample ids]: the forced call runs the same kernel form on the same inputs, so over the
    columns the greedy call produced its logits are the greedy logits byte for byte and its sample_id the greedy ids."""
    bc, w, mode, form = _open(rv, case)
    bc.set_weights_flat(_emitting_flat(rv, bc.cfg, seed=24))      # base-emitting weights: the search runs several steps
    raw, ev = _slab()
    tok, lg = bc.greedy_search_prediction(_x(mode, raw, ev), L)
    tok, lg = tok.numpy().copy(), lg.numpy().copy()
    greedy_forms = _decode_forms(bc)
    S = tok.shape[1]
    assert S >= 2, "the case must decode some steps"
    target = np.full((B, L), PAD, np.int32)
    target[:, 0] = START
    target[:, 1:S + 1] = tok
    r = _forced(bc, mode, raw, ev, target)
    assert _decode_forms(bc) == greedy_forms == {form}, (case, greedy_forms, _decode_forms(bc))
    assert r.logits.shape == (B, L - 1, V)
    assert r.logits[:, :S].tobytes() == lg.tobytes(), (case, "logits differ from the greedy search's", float(np.abs(r.logits[:, :S] - lg).max()))
    assert np.array_equal(r.sample_id[:, :S], tok), case
    bc.close()


# ---------------------------------------------------------------------------------------------- 3: independence of the slab
def test_a_chunk_scores_the_same_in_any_slab(main_case):
    """One chunk and its labels alone, as row 1 of 3 and as row 11 of 17 among other chunks and labels (wide_recurrence at its default):
    logits, nll and sums byte-identical."""
    m = main_case
    bc = m["bc"]
    chunk, labels = 0, m["target"][0:1]
    alone = _forced(bc, "joint", m["raw"][chunk:chunk + 1], m["ev"][chunk:chunk + 1], labels)
    for nB, row in ((3, 1), (17, 11)):
        raw, ev = _slab(nB, seed=40 + nB)
        target = _labels(nB, L, seed=50 + nB)
        raw[row], ev[row], target[row] = m["raw"][chunk], m["ev"][chunk], labels[0]
        r = _forced(bc, "joint", raw, ev, target)
        for name in ("logits", "sample_id", "nll", "nll_sum", "n_labels", "n_match", "n_counted"):
            assert getattr(r, name)[row:row + 1].tobytes() == getattr(alone, name).tobytes(), (nB, name)
    assert alone.logits.tobytes() == _forced(bc, "joint", m["raw"], m["ev"], m["target"]).logits[0:1].tobytes()


# ---------------------------------------------------------------------------------------------- 5: the scoring kernel alone
def _score(bc, logits, labels, omit):
    r = bc.score_logits(labels, logits, omit)
    return type(r)(*[a.numpy() for a in r])


@pytest.mark.parametrize("name,Vv", [(None, 7), ("B", 2), ("A", 8)])
def test_scoring_kernel_alone(rv, name, Vv):
    """rv_score_logits on chosen logits, no decode: ties, equal rows, large magnitudes, all-padding rows, both omit sets, exact counts,
    and nll against fp64 on the same fp32 logits within twice the error of the same formula in numpy float32 + 1e-6."""
    tk = _tokenizer(name) if name else rv.data_loader.nuc_tk
    bc = rv.Basecaller(128, 128, 128, tk, "joint", 0.0, max_batch=8, max_raw_len=TR, max_event_len=TE, max_output_len=64)
    assert bc.cfg.vocab == Vv
    pad, start, end = bc.cfg.pad_token, bc.cfg.start_token, bc.cfg.end_token
    rng = np.random.default_rng(5 + Vv)
    nB, S = 6, 63
    lg = (rng.standard_normal((nB, S, Vv)) * 3).astype(np.float32)
    lab = rng.integers(0, Vv, size=(nB, S)).astype(np.int32)
    lg[0, 0] = 0.25                                           # a row of equal logits: nll = log V, argmax 0
    lg[0, 1, :] = -1.0; lg[0, 1, Vv - 1] = 2.0; lg[0, 1, Vv // 2] = 2.0      # exactly tied maxima: the first wins
    lg[0, 2] = 80.0 * np.where(np.arange(Vv) % 2, -1.0, 1.0)   # magnitude 80: exp(160) overflows float32 without the max subtraction
    lab[0, 2] = 1                                             # ... and the label sits on -80: nll = 160 + log(count of +80)
    lg[0, 3] = -80.0; lg[0, 3, Vv - 1] = 80.0
    lab[1] = pad                                              # an all-padding row
    lg[2] = 0.0                                               # tf.pad's columns: zero logits, id 0
    for omit in ((pad, start, end), (start, end), ()):
        r = _score(bc, lg, lab, omit)
        assert np.array_equal(r.sample_id, np.argmax(lg, -1)), (Vv, "argmax, first maximum on ties")
        assert r.sample_id[0, 1] == Vv // 2 and r.sample_id[0, 0] == 0
        n_match, n_counted = np_counts(lab, r.sample_id, omit)
        assert np.array_equal(r.n_match, n_match) and np.array_equal(r.n_counted, n_counted), (Vv, omit)
        assert np.array_equal(r.n_labels, (lab != pad).sum(-1)) and r.n_labels[1] == 0
    assert np.isfinite(r.nll).all()
    assert (r.nll[lab == pad] == 0).all() and r.nll_sum[1] == 0
    if lab[0, 0] != pad:
        assert abs(r.nll[0, 0] - np.log(Vv)) < 1e-6
    ref = np_nll(lg.astype(np.float64), lab, pad)
    f32 = np_nll(lg, lab, pad)
    assert f32.dtype == np.float32
    e_gpu, e_np = float(np.abs(r.nll - ref).max()), float(np.abs(f32 - ref).max())
    print(f"score kernel V={Vv}: max |nll - fp64| gpu {e_gpu:.2e}, numpy float32 {e_np:.2e}")
    assert e_gpu <= 2 * e_np + 1e-6, (Vv, e_gpu, e_np)
    want = np.zeros(nB, np.float32)
    for s in range(S):
        want = want + r.nll[:, s]
    assert np.array_equal(r.nll_sum, want)
    # loss_function: the quotient of the sums; NaN when every label is padding
    # (its error: the mean of the terms' errors, plus the fp32 sums' -- at most (additions) x 2^-24 x sum |terms|, over the label count)
    loss = float(bc.loss_function(lab, lg))
    assert abs(loss - np_loss(lg.astype(np.float64), lab, pad)) <= (2 * e_np + 1e-6) + (nB * S + nB) * 2.0 ** -24 * ref.sum() / (lab != pad).sum()
    assert np.isnan(float(bc.loss_function(lab[1:2], lg[1:2])))
    # a label outside the vocabulary is refused; S = 0 and B = 0 give empty results
    bad = lab.copy(); bad[3, 5] = Vv
    with pytest.raises(rv._capi.RavventHipError, match="RV_EINVAL"):
        _score(bc, lg, bad, ())
    bad[3, 5] = -1
    with pytest.raises(rv._capi.RavventHipError, match="RV_EINVAL"):
        _score(bc, lg, bad, ())
    e = _score(bc, lg[:, :0], lab[:, :0], ())
    assert e.nll.shape == (nB, 0) and (e.nll_sum == 0).all() and (e.n_labels == 0).all() and (e.n_counted == 0).all()
    assert _score(bc, lg[:0], lab[:0], ()).nll_sum.shape == (0,)
    bc.close()


# ---------------------------------------------------------------------------------------------- 6: end to end
def _partly_right(rv, oracle, bc):
    """Base-emitting weights and label rows the fp64 forced decode gets partly right -> (w, raw, ev, target)."""
    flat = _emitting_flat(rv, bc.cfg, seed=24)
    bc.set_weights_flat(flat)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev = _slab()
    target = _labels(B, L)
    follow = np.random.default_rng(3).random((B, L - 1)) < 0.6
    follow &= (target[:, 1:] != END) & (target[:, 1:] != PAD)          # the early end, its padding and the all-padding row stay
    return w, raw, ev, follow_labels(oracle, w, bc.cfg.oracle_cfg(), raw, ev, target, follow)


def test_evaluate_step_against_the_numpy_restatement(rv, oracle):
    bc, _, mode, _ = _open(rv, "joint")
    w, raw, ev, target = _partly_right(rv, oracle, bc)
    real = target[:, 1:]
    ref, ref_ids = forced_decode(oracle, w, bc.cfg.oracle_cfg(), raw, ev, target)
    twin, _ = forced_decode(oracle, w, bc.cfg.oracle_cfg(), raw, ev, target, dtype=np.float32)
    want_acc = np_masked_accuracy(real, ref_ids, TRAIN_OMIT)
    assert 0 < want_acc < 1, ("the labels must be partly right", want_acc)
    r = _forced(bc, mode, raw, ev, target)
    bound = _bound(r.logits, ref, twin, "evaluate_step")
    _check_scores(r, target, ref, bound, "evaluate_step")
    nll, nll_sum = bc.sequence_nll((raw, ev), target)
    assert nll.numpy().tobytes() == r.nll.tobytes() and nll_sum.numpy().tobytes() == r.nll_sum.tobytes()
    sid, lg = bc.teacher_forced_prediction((raw, ev), target)
    assert sid.numpy().tobytes() == r.sample_id.tobytes() and lg.numpy().tobytes() == r.logits.tobytes()
    got = bc.evaluate_step((raw, ev, target))
    loss, acc = float(got["loss"]), float(got["acc"])
    want_loss = float(np_loss(ref, real))
    print(f"evaluate_step: loss {loss:.7f} (fp64 {want_loss:.7f}), acc {acc:.4f} (fp64 {want_acc:.4f})")
    assert abs(loss - want_loss) <= 2 * bound, (loss, want_loss, bound)          # a mean of terms each within 2 x bound
    assert acc == np_masked_accuracy(real, r.sample_id, TRAIN_OMIT)
    if np.array_equal(r.sample_id, ref_ids):
        assert acc == want_acc
    bc.close()


def test_test_step_pads_an_early_greedy_search(rv, oracle):
    """_val_step on a slab whose greedy search ends early (S < L - 1; base-emitting weights): columns >= S are logits 0 / id 0, the
    padding labels there are counted by the validation omit set and a non-padding label there costs log V."""
    bc, _, mode, _ = _open(rv, "joint", L_max=16)
    flat = _emitting_flat(rv, bc.cfg, seed=24, end_bias=1.35)
    bc.set_weights_flat(flat)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev = _slab()
    Lt = 16
    otok, olg = oracle.greedy_search(w, bc.cfg.oracle_cfg(), raw, ev, Lt)
    twin_tok, twin_lg = oracle.greedy_search(w, bc.cfg.oracle_cfg(), raw, ev, Lt, dtype=np.float32)
    S = otok.shape[1]
    assert 2 <= S < Lt - 1 and np.array_equal(twin_tok, otok), ("the case must end early", S)
    target = np.full((B, Lt), PAD, np.int32)
    target[:, 0] = START
    target[:, 1:S + 1] = otok                       # the search's own calls as labels ...
    target[0, 2] = 3 + (target[0, 2] - 2) % 4       # ... one of them wrong,
    target[1, S + 2] = 4                            # and a base label in the padded columns: its nll is log V
    real = target[:, 1:]
    tok, lg = bc.greedy_search_prediction((raw, ev), Lt)
    assert np.array_equal(tok.numpy(), otok), "the greedy search left the fp64 decode"
    bound = min(TOL, TWIN_K * float(np.abs(twin_lg - olg).max()) + TWIN_C)
    assert float(np.abs(lg.numpy() - olg).max()) <= bound
    pad_lg = np.zeros((B, Lt - 1, V)); pad_lg[:, :S] = olg
    pad_ids = np.zeros((B, Lt - 1), np.int32); pad_ids[:, :S] = otok
    got = bc.test_step((raw, ev, target))
    loss, acc = float(got["loss"]), float(got["acc"])
    print(f"test_step: S {S} of {Lt - 1}, loss {loss:.7f} (fp64 {float(np_loss(pad_lg, real)):.7f}), acc {acc:.4f}")
    assert abs(loss - np_loss(pad_lg, real)) <= 2 * bound
    assert acc == np_masked_accuracy(real, pad_ids, VAL_OMIT) and 0 < acc < 1
    # the padding itself, through the scoring call test_step makes
    gl = np.zeros((B, Lt - 1, V), np.float32); gl[:, :S] = lg.numpy()
    r = bc.score_logits(real, gl, VAL_OMIT)
    assert (r.sample_id.numpy()[:, S:] == 0).all() and abs(float(r.nll[1, S + 1]) - np.log(V)) < 1e-6
    bc.close()


# ---------------------------------------------------------------------------------------------- 7: interface
def test_interface(rv, main_case):
    m = main_case
    bc, raw, ev, target = m["bc"], m["raw"], m["ev"], m["target"]
    # L > max_output_len: the greedy call's message
    msg = {}
    for what, call in (("greedy", lambda: bc.greedy_search_prediction((raw, ev), L + 1)),
                       ("forced", lambda: _forced(bc, "joint", raw, ev, _labels(B, L + 1)))):
        with pytest.raises(rv._capi.RavventHipError) as e:
            call()
        msg[what] = str(e.value).split(": ", 1)[1]
    assert msg["forced"] == msg["greedy"] and "max_output_len" in msg["forced"], msg
    # a target id outside the vocabulary: RV_EINVAL from the host call, whatever its column
    for bad_id, col in ((V, 3), (-1, 0), (V, L - 1)):
        bad = target.copy(); bad[1, col] = bad_id
        with pytest.raises(rv._capi.RavventHipError, match="RV_EINVAL"):
            _forced(bc, "joint", raw, ev, bad)
    # B == 0 and L == 1: empty results, nothing launched
    r = _forced(bc, "joint", raw[:0], ev[:0], target[:0])
    assert r.logits.shape == (0, L - 1, V) and r.nll_sum.shape == (0,) and not _rows(bc, "kernel_forms")
    r = _forced(bc, "joint", raw, ev, target[:, :1])
    assert r.logits.shape == (B, 0, V) and r.sample_id.shape == (B, 0) and not _rows(bc, "kernel_forms")
    assert (r.nll_sum == 0).all() and (r.n_labels == 0).all() and (r.n_match == 0).all() and (r.n_counted == 0).all()
    r = _forced(bc, "joint", raw, ev, target[:, :1], device=True)
    assert r.logits.shape == (B, 0, V) and (r.nll_sum == 0).all() and (r.n_counted == 0).all()
    # a forced call between two asynchronous submits leaves their results as they are without it
    slabs = [_slab(B, seed=60 + i) for i in range(2)]
    want = [tuple(a.numpy().copy() for a in bc.beam_search_prediction(x, 3, L)) for x in slabs]
    ref = _forced(bc, "joint", raw, ev, target)
    bc.set_async_depth(3)
    t0 = bc.submit_beam_search(slabs[0], 3, L)
    mid = _forced(bc, "joint", raw, ev, target)
    t1 = bc.submit_beam_search(slabs[1], 3, L)
    for t, wnt in ((t0, want[0]), (t1, want[1])):
        got = bc.collect(t)
        assert got[0].numpy().tobytes() == wnt[0].tobytes() and got[1].numpy().tobytes() == wnt[1].tobytes()
    for a, b_, name in zip(mid, ref, ref._fields):
        assert a.tobytes() == b_.tobytes(), name
    bc.set_async_depth(2)


@pytest.mark.parametrize("case", ["joint", "two_cells", "per_step", "three_cells"])
def test_device_label_outside_the_vocabulary_adds_no_input_row(rv, case):
    """The device variant cannot check its labels on the host.  With token 0's row of the decoder's input kernel set to zero, feeding 0
    and feeding an id outside [0, V) must be the same arithmetic -- byte-identical logits -- in the persistent and the per-step decode."""
    bc, _, mode, form = _open(rv, case)
    flat = rv.weights.init_weights(bc.cfg, seed=31, gain=1.5)
    flat["dec_cells.0.W"][0] = 0.0
    bc.set_weights_flat(flat)
    raw, ev = _slab()
    target = _labels(B, L)
    target[0, 0], target[1, 3] = 0, 0
    ref = _forced(bc, mode, raw, ev, target, device=True)
    out = target.copy()
    out[0, 0], out[1, 3] = V, -1
    r = _forced(bc, mode, raw, ev, out, device=True)
    assert _decode_forms(bc) == {form}
    assert r.logits.tobytes() == ref.logits.tobytes() and np.array_equal(r.sample_id, ref.sample_id)
    assert np.isnan(r.nll[1, 2]) and np.isfinite(np.delete(r.nll.ravel(), 1 * (L - 1) + 2)).all()       # as a label it has no logit
    bc.close()
