"""CPU side of scoring given label sequences (rv_teacher_forced*, rv_score_logits; Basecaller.teacher_forced_prediction, sequence_nll,
loss_function, evaluate_step, test_step): the numpy restatements the GPU tests hold the kernels to, checked themselves.

  forced_decode   Decoder.call under TrainingSampler (/root/reference/basecaller.py:142-152, :234-244) composed from the oracle's public
                  functions: encode_input, setup_memory and attention_step in a loop over target[:, s] -- greedy_search's loop
                  (oracle/ravvent_oracle.py:258-288) with the label in place of the argmax and no early stop.
  np_nll, np_loss, np_masked_accuracy
                  loss_function (:212-220) and utils.masked_accuracy (/root/reference/utils.py:15-24) in a dozen lines of numpy.
tests/test_teacher_forced_gpu.py imports them from here."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, END, START = 0, 1, 2                    # data_loader.py:20-26
TRAIN_OMIT, VAL_OMIT = (PAD, START, END), (START, END)      # basecaller.py:247, :277


def _forced_loop(oracle, w, cfg, raw, ev, target, dtype, follow=None):
    enc_out, mask = oracle.encode_input(w, raw, ev, cfg["mode"], cfg.get("padding_value", 0.0), dtype)
    keys, values = oracle.setup_memory(w, enc_out, mask, dtype)
    B, d, V = enc_out.shape[0], np.asarray(w["W_att"]).shape[1], np.asarray(w["W_fc"]).shape[1]
    att = np.zeros((B, d), dtype)
    states = [(np.zeros((B, d), dtype), np.zeros((B, d), dtype)) for _ in w["dec_cells"]]
    target = target.copy()
    out = []
    for s in range(target.shape[1] - 1):
        logits, att, _, states = oracle.attention_step(w, target[:, s], att, states, keys, values, mask, cfg["attention_type"], dtype)
        out.append(logits)
        if follow is not None:
            target[:, s + 1] = np.where(follow[:, s], np.argmax(logits, axis=-1), target[:, s + 1])
    lg = np.stack(out, axis=1) if out else np.zeros((B, 0, V), dtype)
    return lg, np.argmax(lg, axis=-1).astype(np.int32), target


def forced_decode(oracle, w, cfg, raw, ev, target, dtype=np.float64):
    """-> (rnn_output logits [B, L-1, V], sample_id [B, L-1]): every step s of every chunk is fed target[:, s]."""
    return _forced_loop(oracle, w, cfg, raw, ev, target, dtype)[:2]


def follow_labels(oracle, w, cfg, raw, ev, target, follow):
    """`target` with the label of step s (target[b, s + 1]) replaced by the fp64 forced decode's own argmax wherever follow[b, s]: label
    rows a model gets partly right, so that an accuracy is neither 0 nor 1."""
    return _forced_loop(oracle, w, cfg, raw, ev, target, np.float64, follow)[2]


def np_nll(logits, labels, pad=PAD):
    """mask * SparseCategoricalCrossentropy(from_logits=True, reduction='none') in the dtype of `logits`, max-subtracted:
    (max - logits[label]) + log(sum(exp(logits - max)))."""
    m = logits.max(-1)
    at = np.take_along_axis(logits, labels[..., None].astype(np.int64), -1)[..., 0]
    nll = (m - at) + np.log(np.exp(logits - m[..., None]).sum(-1, dtype=logits.dtype))
    return np.where(labels != pad, nll, logits.dtype.type(0))


def np_loss(logits, labels, pad=PAD):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np_nll(logits, labels, pad).sum() / np.float64((labels != pad).sum())


def np_counts(y_true, y_pred, omit_vals):
    """-> (n_match, n_counted) per row."""
    mask = np.ones(y_true.shape, bool)
    for ov in omit_vals:
        mask &= y_true != ov
    return (mask & (y_true == y_pred)).sum(-1), mask.sum(-1)


def np_masked_accuracy(y_true, y_pred, omit_vals):
    n_match, n_counted = np_counts(y_true, y_pred, omit_vals)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float64(n_match.sum()) / np.float64(n_counted.sum())


def test_loss_and_accuracy_restatements_on_hand_computed_cases(rv):
    V = 7
    # equal logits: every label costs log V; the padding label costs nothing and is not counted
    labels = np.array([[3, 4, END, PAD]])
    assert np.allclose(np_nll(np.zeros((1, 4, V)), labels), [[np.log(7), np.log(7), np.log(7), 0.0]], rtol=0, atol=1e-15)
    assert abs(np_loss(np.zeros((1, 4, V)), labels) - np.log(7)) < 1e-15
    # probabilities 1/2, 1/4, 1/8, 1/8 on ids 3..6: -log p at the label
    lg = np.full((1, 3, V), -1e9)
    lg[0, :, 3:7] = np.log([0.5, 0.25, 0.125, 0.125])
    lab = np.array([[3, 4, 6]])
    assert np.allclose(np_nll(lg, lab), [[np.log(2), np.log(4), np.log(8)]], rtol=0, atol=1e-12)
    assert abs(np_loss(lg, lab) - np.log(64) / 3) < 1e-12
    # logits of magnitude 80 in float32: the max-subtracted form neither overflows nor loses the small term
    big = np.array([[[80.0, -80.0, 79.0, 0, 0, 0, 0]]], np.float32)
    assert np.isfinite(np_nll(big, np.array([[1]]))).all()
    assert abs(np_nll(big, np.array([[1]]))[0, 0] - (160.0 + np.log1p(np.exp(-1.0)))) < 2e-5
    # masked_accuracy, both omit sets: labels $ a c ^ '' '' against predictions $ a g ^ '' ''
    y_true = np.array([[START, 3, 4, END, PAD, PAD]])
    y_pred = np.array([[START, 3, 5, END, PAD, PAD]])
    assert np_counts(y_true, y_pred, TRAIN_OMIT) == (1, 2) and np_masked_accuracy(y_true, y_pred, TRAIN_OMIT) == 0.5
    assert np_counts(y_true, y_pred, VAL_OMIT) == (3, 4) and np_masked_accuracy(y_true, y_pred, VAL_OMIT) == 0.75       # the padding counts
    assert rv.utils.masked_accuracy(y_true, y_pred, TRAIN_OMIT) == 0.5 and rv.utils.masked_accuracy(y_true, y_pred, VAL_OMIT) == 0.75
    # all padding: 0 / 0, as the reference's divisions give; the validation form still counts the padding labels
    allpad = np.zeros((2, 5), np.int64)
    assert np.isnan(np_loss(np.zeros((2, 5, V)), allpad)) and np.isnan(np_masked_accuracy(allpad, allpad, TRAIN_OMIT))
    assert np.isnan(rv.utils.masked_accuracy(allpad, allpad, TRAIN_OMIT))
    assert np_masked_accuracy(allpad, allpad, VAL_OMIT) == 1.0 and (np_nll(np.zeros((2, 5, V)), allpad) == 0).all()


def test_forced_loop_fed_the_greedy_ids_is_the_greedy_search(rv, oracle):
    """Teacher forcing with target = [start | the greedy search's own ids] IS the greedy search: the composed loop reproduces
    oracle.greedy_search's logits exactly in fp64, for every attention type and a stacked decoder."""
    raw, ev, _ = rv.synthetic.make_slab(3, 14, 5, seed=4)
    for attention, depth in (("luong", 1), ("bahdanau", 1), ("luong", 2)):
        cfg = rv.RvConfig(enc_units=16, dec_units=16, enc_depth=2, dec_depth=depth, attention=attention)
        flat = rv.weights.init_weights(cfg, seed=5, gain=2.0)
        flat["b_fc"][cfg.end_token] -= 4.0                      # no chunk ends early: the greedy loop runs all L - 1 steps
        w = rv.weights.flat_to_nested(cfg, flat)
        L = 7
        ids, lg = oracle.greedy_search(w, cfg.oracle_cfg(), raw, ev, L)
        assert ids.shape[1] == L - 1, "the case must run every step"
        target = np.concatenate([np.full((3, 1), cfg.start_token, np.int32), ids], axis=1)
        flg, fid = forced_decode(oracle, w, cfg.oracle_cfg(), raw, ev, target)
        assert np.array_equal(flg, lg) and np.array_equal(fid, ids), (attention, depth)
        # and it is the labels that are fed, not the argmax: other labels give other logits from step 1 on, the same at step 0
        other = target.copy()
        other[:, 1:] = 3 + (other[:, 1:] - 2) % 4          # another base letter in every column
        olg, _ = forced_decode(oracle, w, cfg.oracle_cfg(), raw, ev, other)
        assert np.array_equal(olg[:, 0], lg[:, 0]) and not np.array_equal(olg[:, 1], lg[:, 1])


def test_new_symbols_are_declared_and_bound(rv):
    hdr = open(os.path.join(ROOT, "include", "ravvent_hip.h")).read()
    bound = {n: args for n, _, args in rv._capi.SYMBOLS}
    for name, nargs in (("rv_teacher_forced", 12), ("rv_teacher_forced_dev", 12), ("rv_score_logits", 8)):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M)
        assert m, f"{name} is not declared in include/ravvent_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(bound[name]), name
    m = re.search(r"typedef struct RvScore \{([^}]*)\} RvScore;", hdr)
    fields = [f.split("*")[-1].strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == [n for n, _ in rv._capi.CRvScore._fields_] == ["nll", "nll_sum", "n_labels", "n_match", "n_counted"]
    assert re.search(r"#define RV_ABI_VERSION 1\b", hdr), "adding entry points keeps the ABI version"
    for method in ("teacher_forced_prediction", "sequence_nll", "loss_function", "evaluate_step", "test_step"):
        assert callable(getattr(rv.Basecaller, method))
