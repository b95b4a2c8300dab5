"""The BiGRU family in numpy (fp64 = reference of record, fp32 = its twin) -- TEST INFRASTRUCTURE, NOT PRODUCT.

Keras GRUCell with the TF >= 2.7 defaults the reference's rnn_type 'bigru' builds (basecaller.py:18-46, 85-89): reset_after=True,
sigmoid / tanh, gate order z, r, h.  Per cell W [F,3u], U [u,3u], b [2,3u] (row 0 the input bias, row 1 the recurrent bias):

    xi = x.W + b[0]               hr = h.U + b[1]
    z  = sigmoid(xi_z + hr_z)     r  = sigmoid(xi_r + hr_r)
    hh = tanh(xi_h + r * hr_h)    h' = z * h + (1 - z) * hh

tests/test_gru.py holds these formulas to torch.nn.GRU(bidirectional=True) in fp64.  encode_input, attention_step, greedy_search and
beam_search take the signatures and fill the tap names of oracle/ravvent_oracle.py, so the helpers of tests/test_parity_gpu.py
(_greedy_errors, _beam_errors, _twin_greedy, _twin_beam, _assert_twin) take this module in place of their `oracle` argument.
Everything that does not depend on the cell comes from the oracle; only the cell, the layers built of it and the loops that carry a
state of h alone are stated here.  The product never imports this module.
"""
import numpy as np

from oracle.ravvent_oracle import (F32_MIN, _sigmoid, beam_search_step, gather_tree, input_mask, log_softmax,  # noqa: F401  (log_softmax: part of the oracle's surface the helpers may ask for)
                                   setup_memory, tokens_to_nuc_sequences)  # noqa: F401


def gru_cell(x, h, W, U, b):
    u = h.shape[-1]
    xi = x @ W + b[0]
    hr = h @ U + b[1]
    z = _sigmoid(xi[..., :u] + hr[..., :u])
    r = _sigmoid(xi[..., u:2 * u] + hr[..., u:2 * u])
    hh = np.tanh(xi[..., 2 * u:] + r * hr[..., 2 * u:])
    return z * h + (1 - z) * hh


def bigru_layer(x, fwd, bwd, init):
    """Bidirectional(RNN(GRUCell, return_sequences, return_state)), merge 'concat'; init None (zeros) or (h_f, h_b).  No mask."""
    B, T, _ = x.shape
    u = fwd[1].shape[0]
    dt = x.dtype
    hf, hb = (np.zeros((B, u), dt), np.zeros((B, u), dt)) if init is None else [a.astype(dt) for a in init]
    out = np.empty((B, T, 2 * u), dt)
    for t in range(T):
        hf = gru_cell(x[:, t], hf, *fwd)
        out[:, t, :u] = hf
    for t in range(T - 1, -1, -1):
        hb = gru_cell(x[:, t], hb, *bwd)
        out[:, t, u:] = hb
    return out, (hf, hb)


def encoder(x, layers):
    """Encoder.call (basecaller.py:48-59): layer l+1 starts from layer l's two final states; layer 0 from zeros."""
    states, out = None, x
    for lw in layers:
        out, states = bigru_layer(out, lw["fwd"], lw["bwd"], states)
    return out, states


def _cast_layers(layers, dtype):
    return [{d: tuple(np.asarray(a, dtype) for a in lw[d]) for d in ("fwd", "bwd")} for lw in layers]


def encode_input(weights, raw, event, mode, padding_value=0.0, dtype=np.float64):
    outs, masks = [], []
    if mode in ("raw", "joint"):
        r = np.asarray(raw, dtype)
        masks.append(input_mask(r, padding_value))
        outs.append(encoder(r, _cast_layers(weights["enc_raw"], dtype))[0])
    if mode in ("event", "joint"):
        e = np.asarray(event, dtype)
        masks.append(input_mask(e, padding_value))
        outs.append(encoder(e, _cast_layers(weights["enc_event"], dtype))[0])
    return np.concatenate(outs, axis=1), np.concatenate(masks, axis=1)


def attention_step(weights, tok, att_prev, cell_states, keys, values, mask, attention_type, dtype):
    """One AttentionWrapper step over StackedRNNCells of GRUCell + the output layer; cell_states: one h per cell.
    returns logits, att, alpha, new_cell_states"""
    V = np.asarray(weights["W_fc"]).shape[1]
    x = np.concatenate([np.eye(V, dtype=dtype)[tok], att_prev], axis=-1)
    new_states = []
    for h, cw in zip(cell_states, weights["dec_cells"]):
        x = gru_cell(x, h, *(np.asarray(a, dtype) for a in cw))
        new_states.append(x)
    q = x
    if attention_type == "luong":
        score = np.einsum("...d,...td->...t", q, keys)
    elif attention_type == "bahdanau":
        pq = q @ np.asarray(weights["W_q"], dtype)
        score = np.sum(np.asarray(weights["v_att"], dtype) * np.tanh(keys + pq[..., None, :]), axis=-1)
    else:
        raise ValueError(attention_type)
    score = np.where(mask, score, -np.inf)
    with np.errstate(invalid="ignore"):                   # an all-padding chunk: NaN alignments, as the layers give
        e = np.exp(score - np.max(score, axis=-1, keepdims=True))
        alpha = e / np.sum(e, axis=-1, keepdims=True)
    ctx = np.einsum("...t,...te->...e", alpha, values)
    att = np.concatenate([q, ctx], axis=-1) @ np.asarray(weights["W_att"], dtype)
    logits = att @ np.asarray(weights["W_fc"], dtype) + np.asarray(weights["b_fc"], dtype)
    return logits, att, alpha, new_states


def beam_search(weights, cfg, raw, event, beam_width, max_output_len, dtype=np.float64, taps=None):
    W = int(beam_width)
    end, start = cfg["end_token"], cfg["start_token"]
    enc_out, mask = encode_input(weights, raw, event, cfg["mode"], cfg.get("padding_value", 0.0), dtype)
    keys, values = setup_memory(weights, enc_out, mask, dtype)
    B = enc_out.shape[0]
    d = np.asarray(weights["W_att"]).shape[1]
    keys_b, values_b, mask_b = keys[:, None], values[:, None], mask[:, None]
    tok = np.full((B, W), start, np.int32)
    att = np.zeros((B, W, d), dtype)
    states = [np.zeros((B, W, d), dtype) for _ in weights["dec_cells"]]
    log_probs = np.full((B, W), -np.inf, dtype)
    log_probs[:, 0] = 0.0
    finished = np.zeros((B, W), bool)
    lengths = np.zeros((B, W), np.int64)
    ids, parents, scores, all_logits, all_align = [], [], [], [], []
    for _ in range(int(max_output_len) - 1):
        if finished.all():
            break
        logits, att_new, alpha, new_states = attention_step(weights, tok, att, states, keys_b, values_b, mask_b, cfg["attention_type"], dtype)
        top, word, parent, log_probs, finished, lengths = beam_search_step(logits, log_probs, finished, lengths, end)
        g = lambda a: np.take_along_axis(a, parent[..., None], axis=1)
        att = g(att_new)
        states = [g(h) for h in new_states]
        tok = word if not finished.all() else np.full((B, W), start, np.int32)
        ids.append(word); parents.append(parent); scores.append(top)
        all_logits.append(logits); all_align.append(alpha)
    if not ids:
        return np.zeros((B, 0), np.int32), np.zeros((B, 0), dtype)
    step_ids, parent_ids = np.stack(ids), np.stack(parents)
    pred = gather_tree(step_ids, parent_ids, lengths.max(axis=1).astype(np.int32), end)
    if taps is not None:
        taps.update(enc_output=enc_out, mask=mask, keys=keys, step_logits=np.stack(all_logits), step_alignments=np.stack(all_align),
                    step_ids=step_ids, parent_ids=parent_ids, lengths=lengths, finished=finished, step_scores=np.stack(scores),
                    log_probs=log_probs, predicted_ids=pred)
    return np.transpose(pred, (1, 0, 2))[:, :, 0].astype(np.int32), np.transpose(np.stack(scores), (1, 0, 2))[:, :, 0]


def greedy_search(weights, cfg, raw, event, max_output_len, dtype=np.float64, taps=None, forced=None):
    """forced [B,L] (None: the argmax feeds back): step s feeds forced[:, s] and every chunk runs L - 1 steps (TrainingSampler)."""
    end, start = cfg["end_token"], cfg["start_token"]
    enc_out, mask = encode_input(weights, raw, event, cfg["mode"], cfg.get("padding_value", 0.0), dtype)
    keys, values = setup_memory(weights, enc_out, mask, dtype)
    B = enc_out.shape[0]
    d = np.asarray(weights["W_att"]).shape[1]
    tok = np.full((B,), start, np.int32) if forced is None else np.asarray(forced)[:, 0].astype(np.int32)
    att = np.zeros((B, d), dtype)
    states = [np.zeros((B, d), dtype) for _ in weights["dec_cells"]]
    finished = np.zeros((B,), bool)
    ids, all_logits, all_align = [], [], []
    for s in range(int(max_output_len) - 1):
        if forced is None and finished.all():
            break
        logits, att, alpha, states = attention_step(weights, tok, att, states, keys, values, mask, cfg["attention_type"], dtype)
        sample = np.argmax(logits, axis=-1).astype(np.int32)
        finished = finished | (sample == end)
        tok = sample if forced is None else np.asarray(forced)[:, s + 1].astype(np.int32)
        ids.append(sample); all_logits.append(logits); all_align.append(alpha)
    if taps is not None:
        taps.update(enc_output=enc_out, mask=mask, keys=keys, step_alignments=np.stack(all_align) if all_align else None)
    if not ids:
        V = np.asarray(weights["W_fc"]).shape[1]
        return np.zeros((B, 0), np.int32), np.zeros((B, 0, V), dtype)
    return np.stack(ids, axis=1), np.stack(all_logits, axis=1)
