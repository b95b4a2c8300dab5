"""The tie rule of the beam step -- top W of W * V candidates, ties to the lowest flat index beam * V + token (tf.math.top_k) -- on
ties that are exact in every arithmetic, against an integer model with no floating point.

Construction.  With W_fc = 0 and b_fc = c the logits of every beam of every chunk at every step are exactly c.  c holds HIGH (0.25) on
a set H of tokens and LOW (-1.0e4) on the rest: exp(LOW - HIGH) is exactly 0 in fp32 and fp64, so every H token's log-probability is
the same number p = -ln|H| in every beam, a hypothesis's score is p added n times in the same order -- bit-identical for all
hypotheses with the same n -- and hypotheses with different n are ln|H| apart.  The whole decode is decided by (n, flat index) alone.

The model (tie_model) keeps per beam: dead (score -inf) or alive with n live steps, finished, length.  A candidate's key is its class
and n: class 3 real (a live beam's H token at n + 1, a finished beam's end token at its own n), class 2 a live beam's LOW token,
class 1 a finished beam's other tokens (the -FLT_MAX row of _mask_probs), class 0 a dead beam's.  A stable sort selects; the model
raises when a class 1 or 2 candidate is selected, since such a case would depend on the arithmetic: the case is then badly chosen.
With |H| >= W that never happens; class 0 is selected only at step 0 of V < W (fewer real candidates than beams), where the -inf
fillers tie exactly too.

Here, on the CPU, every restatement of the rule must reproduce the model exactly: oracle.beam_search in fp64, its numpy fp32 twin,
oracle/torch_eager.py (records through its taps), and the C port (top-1 tokens of the fp64 pass, scores within 1e-4; one decoder cell
only).  tests/test_exact_ties_gpu.py holds every decode form of the GPU to the same model."""
import numpy as np
import pytest

HIGH, LOW = 0.25, -1.0e4
TOL = 1e-4
B, TR, TE, L = 3, 40, 8, 12

# name -> (vocab, start, end, pad, input padding value): the reference's own ids, and configurations A and E of test_config_space_gpu
CONFIGS = {
    "default": (7, 2, 1, 0, 0.0),
    "A": (8, 7, 0, 3, -1.0),      # W * V = 64 candidates at beam 8, a full wave; end token 0: the first lane of every beam
    "E": (8, 0, 7, 7, 0.0),       # end token 7: the last lane of every beam
}
ALL = None                        # H = every token
HOLES = ((1, 3, 4, 6), (3, 4, 5, 6))     # maxima in non-adjacent lanes, end token inside; nothing ever finishes

# (configuration, H, W, attention, decoder cells)
CASES = [("default", ALL, W, "luong", 1) for W in (1, 2, 3, 5, 7, 8)] + \
        [("default", H, W, "luong", 1) for H in HOLES for W in (1, 2, 4)] + \
        [("default", (6,), 1, "luong", 1)] + \
        [(c, ALL, W, "luong", 1) for c in ("A", "E") for W in (1, 3, 5, 8)] + \
        [("default", ALL, 5, "luong", 2), ("default", ALL, 8, "bahdanau", 1)]


def case_id(case):
    name, H, W, attention, D = case
    return f"{name}-H{'all' if H is None else ''.join(map(str, H))}-W{W}-{attention}{D}"


def tokens_of(V, H):
    return tuple(range(V)) if H is None else tuple(H)


class BadlyChosen(Exception):
    """The model selected a candidate whose rank depends on the arithmetic."""


def tie_model(V, end, H, W, L):
    """-> dict(step_ids, parent_ids, n [S, W] (live steps behind each slot's score, -1: a dead beam), lengths, finished [W], S)."""
    H = set(tokens_of(V, H))
    flat_scores = len(H) == 1                  # p = -ln 1 = 0: every real candidate has the same score whatever its n
    dead, n, fin, ln = [w > 0 for w in range(W)], [0] * W, [False] * W, [0] * W
    ids, par, ns = [], [], []
    for _ in range(L - 1):
        if all(fin):
            break
        keys = []
        for w in range(W):
            for v in range(V):
                if dead[w]:
                    keys.append((0, 0))
                elif fin[w]:
                    keys.append((3, n[w]) if v == end else (1, 0))
                else:
                    keys.append((3, n[w] + 1) if v in H else (2, 0))
        rank = lambda k: (-k[0], 0 if flat_scores else k[1])
        top = sorted(range(W * V), key=lambda i: rank(keys[i]))[:W]             # sorted() is stable: ties keep the lowest flat index
        for i in top:
            if keys[i][0] in (1, 2):
                raise BadlyChosen(f"candidate {i} of class {keys[i][0]} selected at step {len(ids)}")
        word, parent = [i % V for i in top], [i // V for i in top]
        new = [(dead[p], keys[i][1], fin[p] or v == end, ln[p] + (0 if fin[p] else 1)) for i, v, p in zip(top, word, parent)]
        dead, n, fin, ln = (list(t) for t in zip(*new))
        ids.append(word); par.append(parent); ns.append([-1 if d else k for d, k in zip(dead, n)])
    a = lambda x: np.asarray(x, np.int64).reshape(len(ids), W)
    return dict(step_ids=a(ids), parent_ids=a(par), n=a(ns), lengths=np.asarray(ln, np.int64), finished=np.asarray(fin), S=len(ids))


def model_scores(m, V, H):
    """n * (-ln|H|) in fp64 for every slot of the model's records [S, W]; -inf for a dead beam."""
    return np.where(m["n"] < 0, -np.inf, m["n"] * -np.log(float(len(tokens_of(V, H)))))


def greedy_model(V, end, H, L):
    """(token, S) of the greedy sampler: argmax takes the first maximum, min(H), at every step; the loop stops once it is the end token."""
    t = min(tokens_of(V, H))
    return t, 1 if t == end else L - 1


def tie_flat(rv, cfg, H, seed=5):
    """init_weights(seed) with the output layer replaced: W_fc = 0, b_fc = HIGH on H and LOW elsewhere."""
    flat = rv.weights.init_weights(cfg, seed=seed)
    flat["W_fc"] = np.zeros_like(flat["W_fc"])
    b = np.full(cfg.vocab, LOW, np.float32)
    b[list(tokens_of(cfg.vocab, H))] = HIGH
    flat["b_fc"] = b
    return flat


def tie_slab(rv, pad=0.0):
    """Three different chunks, the second with suffix padding in the handle's own padding value."""
    raw, ev, _ = rv.synthetic.make_slab(B, TR, TE, seed=0, max_raw_pad=0, max_event_pad=0)
    raw[1, TR - 9:] = pad
    ev[1, TE - 2:] = pad
    return raw, ev


def _cfg(rv, name, attention, D):
    V, start, end, pad_token, pad = CONFIGS[name]
    return rv.RvConfig(attention=attention, dec_depth=D, vocab=V, start_token=start, end_token=end, pad_token=pad_token, padding_value=pad)


def assert_records(t, m, tag):
    """Records [S, B, W] / [B, W] of one restatement against the model's, identically for every chunk."""
    assert t["step_ids"].shape[0] == m["S"], (tag, "S", t["step_ids"].shape[0], m["S"])
    for k in ("step_ids", "parent_ids"):
        assert (np.asarray(t[k]) == m[k][:, None]).all(), (tag, k, np.asarray(t[k])[:, 0].tolist(), m[k].tolist())
    assert (np.asarray(t["lengths"]) == m["lengths"][None]).all(), (tag, "lengths", np.asarray(t["lengths"])[0].tolist(), m["lengths"].tolist())
    assert (np.asarray(t["finished"]) == m["finished"][None]).all(), (tag, "finished")


# the cases the model is known by: hand-checked records
def test_model_micro_cases():
    m = tie_model(7, 1, ALL, 5, L)                                      # one beam finishes per step; the chunk runs all L - 1 steps
    assert m["parent_ids"][:3].tolist() == [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 2, 1, 1, 1]] and m["S"] == L - 1
    assert m["parent_ids"][3].tolist() == [0, 1, 3, 2, 2] and m["lengths"].tolist() == [1, 2, 3, 4, 11]
    m = tie_model(8, 0, ALL, 8, L)                                      # 64 tied candidates; all beams finished after step 8
    assert m["S"] == 8 and m["lengths"].tolist() == list(range(1, 9))
    m = tie_model(8, 7, ALL, 8, L)                                      # lane 7 is the end token
    assert m["step_ids"][0].tolist() == list(range(8)) and m["parent_ids"][1].tolist() == [7, 0, 0, 0, 0, 0, 0, 0]
    m = tie_model(7, 1, (1, 3, 4, 6), 4, L)
    assert m["step_ids"][0].tolist() == [1, 3, 4, 6] and m["S"] == 4
    m = tie_model(7, 1, (3, 4, 5, 6), 4, L)                             # nothing ever finishes, the parents are all 0
    assert m["S"] == L - 1 and not m["parent_ids"].any() and not m["finished"].any()
    m = tie_model(7, 1, ALL, 8, L)                                      # V < W: the eighth slot of step 0 is the first -inf filler, lane 7
    assert (m["step_ids"][0, 7], m["parent_ids"][0, 7], m["n"][0, 7]) == (0, 1, -1)
    with pytest.raises(BadlyChosen):                                    # |H| < W: a LOW token would be selected
        tie_model(7, 1, (3, 4), 3, L)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cpu_restatements_follow_the_model(rv, oracle, case):
    from oracle import cpu_port, torch_eager
    name, H, W, attention, D = case
    cfg = _cfg(rv, name, attention, D)
    V, end = cfg.vocab, cfg.end_token
    flat = tie_flat(rv, cfg, H)
    w, ocfg = rv.weights.flat_to_nested(cfg, flat), cfg.oracle_cfg()
    raw, ev = tie_slab(rv, cfg.padding_value)
    m = tie_model(V, end, H, W, L)
    want = model_scores(m, V, H)
    mtok = oracle.gather_tree(m["step_ids"][:, None], m["parent_ids"][:, None], [int(m["lengths"].max())], end)[:, 0, 0]
    t64 = {}
    tok64, sc64 = oracle.beam_search(w, ocfg, raw, ev, W, L, dtype=np.float64, taps=t64)
    assert_records(t64, m, "fp64")
    assert (t64["step_logits"] == flat["b_fc"].astype(np.float64)).all(), "fp64 logits are not the bias"
    assert (tok64 == mtok[None]).all() and np.abs(sc64 - want[None, :, 0]).max() < 1e-12
    t32 = {}
    tok32, sc32 = oracle.beam_search(w, ocfg, raw, ev, W, L, dtype=np.float32, taps=t32)
    assert_records(t32, m, "fp32 twin")
    assert (tok32 == tok64).all() and np.abs(sc32 - sc64).max() < TOL
    tt = {}
    ttok, tsc = torch_eager.beam_search(w, ocfg, raw, ev, W, L, taps=tt)
    assert_records(tt, m, "torch_eager")
    assert (ttok == tok64).all() and np.abs(tsc - sc64).max() < TOL
    if D == 1:
        ctok, csc = cpu_port.run(dict(ocfg, pad_token=cfg.pad_token), cfg.enc_depth, V, rv.weights.pack(cfg, flat), raw, ev, W, L)
        assert ctok.shape == tok64.shape and (ctok == tok64).all(), ("C port", ctok.tolist(), tok64.tolist())
        assert np.abs(csc - sc64).max() < TOL
    # greedy: min(H) at every step
    gt, gS = greedy_model(V, end, H, L)
    for dt in (np.float64, np.float32):
        g, lg = oracle.greedy_search(w, ocfg, raw, ev, L, dtype=dt)
        assert g.shape == (B, gS) and (g == gt).all(), (dt, g.tolist(), gt, gS)
        assert (lg == flat["b_fc"].astype(dt)).all()
    if D == 1:
        cg, clg = cpu_port.run(dict(ocfg, pad_token=cfg.pad_token), cfg.enc_depth, V, rv.weights.pack(cfg, flat), raw, ev, 1, L, greedy=True)
        assert cg.shape == (B, gS) and (cg == gt).all() and (clg == flat["b_fc"]).all()
