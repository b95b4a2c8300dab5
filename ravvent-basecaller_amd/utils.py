"""Hot-path helpers the reference's callers take from its `utils` module
(/root/reference/ravvent_performance_evaluator.py:53,66)."""
from __future__ import annotations

import numpy as np


def input_mask(input_sequence, padding_value):
    """/root/reference/utils.py:26-32 -- True where EVERY feature of a timestep differs from the
    padding value.  (On the GPU path this is folded into the encoder kernels; this host form
    exists for callers and tests.)"""
    return np.all(np.asarray(input_sequence) != padding_value, axis=-1)


def unpack_data_to_input_target(data, input_data_type):
    """/root/reference/utils.py:34-43"""
    raw_sequence, events_sequence, target_sequence = data
    if input_data_type == "raw":
        return raw_sequence, target_sequence
    if input_data_type == "event":
        return events_sequence, target_sequence
    if input_data_type == "joint":
        return (raw_sequence, events_sequence), target_sequence
    raise ValueError(f"input_data_type {input_data_type!r}")


def masked_accuracy(y_true, y_pred, omit_vals):
    """/root/reference/utils.py:15-24 -- the share of the labels outside `omit_vals` that `y_pred` equals (NaN when there is none).
    Host form; Basecaller.evaluate_step / test_step take the same counts from the GPU (rv_teacher_forced, rv_score_logits)."""
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    mask = np.ones(y_true.shape, bool)
    for ov in omit_vals:
        mask &= y_true != ov
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float64((mask & (y_true == y_pred)).sum()) / np.float64(mask.sum())


def calc_prob_logits_beam_search_scores(beam_scores):
    """/root/reference/utils.py:123-128 -- exp(score_t - score_{t-1}), score_{-1} = 0, along the
    last axis.  Accepts numpy arrays or torch tensors (host or device); returns the same kind."""
    try:
        import torch
        if isinstance(beam_scores, torch.Tensor):
            prev = torch.zeros_like(beam_scores)
            prev[..., 1:] = beam_scores[..., :-1]
            return torch.exp(beam_scores - prev)
    except ImportError:  # pragma: no cover
        pass
    s = np.asarray(beam_scores)
    prev = np.zeros_like(s)
    prev[..., 1:] = s[..., :-1]
    return np.exp(s - prev)


def calc_prob_path_scores(path_scores):
    """Per-base probabilities of every hypothesis of a beam: exp(p_t - p_{t-1}), p_{-1} = 0, along axis 1 of
    `BeamHypotheses.path_scores` [B,S,W] (Basecaller.beam_search_hypotheses) -- the probability of tokens[b, t, w] given that
    hypothesis's own prefix.  (calc_prob_logits_beam_search_scores on scores[:, :, 0] takes slot 0's score at every step, which is
    another hypothesis's wherever the best path did not sit in slot 0.)  Accepts numpy arrays or torch tensors; returns the same kind."""
    try:
        import torch
        if isinstance(path_scores, torch.Tensor):
            prev = torch.zeros_like(path_scores)
            prev[:, 1:] = path_scores[:, :-1]
            return torch.exp(path_scores - prev)
    except ImportError:  # pragma: no cover
        pass
    s = np.asarray(path_scores)
    prev = np.zeros_like(s)
    prev[:, 1:] = s[:, :-1]
    return np.exp(s - prev)
