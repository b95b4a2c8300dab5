"""GPU parity tests proper: the HIP path, called through the C-ABI (ctypes) behind the
`Basecaller` API, against the CPU oracle on the same seeded inputs.

Tolerances (BASELINE.json north_star): base-call strings bit-exact at beam=1, attention /
logit tensors within 1e-4 (fp32) of the fp64 oracle; and, beside that acceptance bar, every tapped tensor no further from fp64 than
TWIN_K x the oracle's numpy fp32 twin + TWIN_C (_assert_twin below)."""
import numpy as np
import pytest

from test_bench_config_gpu import TWIN_C, TWIN_K, _agreeing_steps

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _mk(rv, mode="joint", attention="luong", enc_depth=2, seed=22, gain=1.0, **kw):
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=enc_depth,
                       attention_type=attention, honor_attention_type=True, max_batch=kw.pop("max_batch", 64),
                       **kw)
    flat = bc.init_random_weights(seed=seed, gain=gain)
    return bc, rv.weights.flat_to_nested(bc.cfg, flat)


def _inputs(rv, mode, raw, ev):
    return {"joint": (raw, ev), "raw": raw, "event": ev}[mode]


def _check_alignments(al, ref, mask, cs, tag, last=None):
    """Alignments tapped from the persistent decode (option persist_taps), al [S, B, W, T_m], against the fp64 oracle's ref
    [S', B, W, T_m], on every step each chunk ran (cs = chunk_steps; `last` caps the steps compared): within 1e-4, exactly 0.0 on
    the masked memory steps, summing to 1 within 1e-5.  Returns the largest error."""
    worst = 0.0
    for b in range(al.shape[1]):
        n = int(cs[b]) if last is None else min(int(cs[b]), int(last[b]))
        if n == 0:
            continue
        a = al[:n, b]
        assert np.isfinite(a).all(), (tag, b)
        err = float(np.abs(a - ref[:n, b]).max())
        worst = max(worst, err)
        assert err < TOL, (tag, b, err)
        assert (a[..., mask[b] == 0] == 0.0).all(), (tag, b, "masked step with a non-zero alignment")
        assert np.abs(a.astype(np.float64).sum(-1) - 1.0).max() < 1e-5, (tag, b)
    return worst


# ----------------------------------------------------------------------------------------------
# The twin-relative bound.  1e-4 is the acceptance bar, not what fp32 arithmetic gives: the oracle's own numpy fp32 twin sits at
# 1e-9 (alignments) to 3e-7 (logits) from its fp64 pass on these cases, so a kernel a hundred times less precise than it is would
# still pass `< TOL`.  Beside every fp64 comparison of a tapped tensor the tests therefore run the oracle once more with
# dtype = np.float32 on the same weights and inputs and hold the GPU to
#     max |gpu - fp64| <= TWIN_K x max |twin - fp64| + TWIN_C
# per tensor, each side over the steps on which IT still agrees with the fp64 decode.  TWIN_K and TWIN_C are the constants of the
# adversarial tests (test_bench_config_gpu): "no further from fp64 than an honest fp32 evaluation"; they come from the reference
# side only and do not move towards what the kernels measure (measured values: DESIGN.md section 5).
def _beam_errors(lg, al, ids, par, cs, sc, o, osc):
    """{tensor: max |x - fp64|} of one beam search against the fp64 pass (taps o, top-1 scores osc), and the chunks that left it.
    Step logits lg [S, B, W, V] and alignments al [S, B, W, T_m] (None: not tapped) over every step up to the first one whose beam
    ids or parents differ (_agreeing_steps; cs: the steps each chunk ran), alignments on the unmasked memory steps; the top-1 scores
    sc [B, S] (None: not compared) on the chunks that never left."""
    So, nB = o["step_ids"].shape[0], ids.shape[1]
    n = _agreeing_steps(ids, par, o["step_ids"], o["parent_ids"], cs)
    live = np.asarray(o["mask"]) != 0
    err = dict(step_logits=0.0)
    if al is not None:
        err["step_alignments"] = 0.0
    if sc is not None:
        err["scores"] = 0.0
    left = []
    for b in range(nB):
        m = min(int(cs[b]), So)
        if ((ids[:m, b] != o["step_ids"][:m, b]) | (par[:m, b] != o["parent_ids"][:m, b])).any():
            left.append(b)
        elif sc is not None:
            S = min(sc.shape[1], osc.shape[1])
            err["scores"] = max(err["scores"], float(np.abs(sc[b, :S] - osc[b, :S]).max(initial=0.0)))
        k = int(n[b])
        if k:
            err["step_logits"] = max(err["step_logits"], float(np.abs(lg[:k, b] - o["step_logits"][:k, b]).max()))
            if al is not None:
                d = np.abs(al[:k, b][..., live[b]] - o["step_alignments"][:k, b][..., live[b]])
                err["step_alignments"] = max(err["step_alignments"], float(d.max(initial=0.0)))
    return err, left


def _greedy_errors(tok, lg, al, og, olg, o):
    """The same for a greedy search: logits lg [B, S, V] and alignments al [S, B, T_m] (None: not tapped) up to and including each
    chunk's first token that differs from the fp64 decode's (og, olg, taps o)."""
    S = min(tok.shape[1], og.shape[1])
    live = np.asarray(o["mask"]) != 0
    err = dict(step_logits=0.0)
    if al is not None:
        err["step_alignments"] = 0.0
    left = []
    for b in range(tok.shape[0]):
        diff = np.nonzero(tok[b, :S] != og[b, :S])[0]
        k = int(diff[0]) + 1 if diff.size else S
        if diff.size:
            left.append(b)
        if k:
            err["step_logits"] = max(err["step_logits"], float(np.abs(lg[b, :k] - olg[b, :k]).max()))
            if al is not None:
                d = np.abs(al[:k, b][..., live[b]] - o["step_alignments"][:k, b][..., live[b]])
                err["step_alignments"] = max(err["step_alignments"], float(d.max(initial=0.0)))
    return err, left


def _memory_errors(enc, keys, o, rows=slice(None)):
    """{enc_output, keys: max |x - fp64|} of the encoder output [B, T_m, 2u] and the attention keys [B, T_m, d] (None: left out)."""
    err = {}
    if enc is not None:
        err["enc_output"] = float(np.abs(enc - o["enc_output"][rows]).max())
    if keys is not None:
        err["keys"] = float(np.abs(keys - o["keys"][rows]).max())
    return err


def _stays(left, nB, tag):
    """A case only probes the decode while the fp32 twin itself stays on the fp64 decode: on at least three quarters of the chunks
    (the cap the adversarial tests put on near-tie chunks), else its inputs must change."""
    assert len(left) <= nB // 4, (tag, "a poor probe: the numpy fp32 twin leaves the fp64 decode on chunks", left)


def _twin_beam(oracle, w, cfg, raw, ev, W, L, o, osc, tag):
    """One pass of the oracle's numpy fp32 twin over a beam search whose fp64 pass gave (o, osc): its error dict against fp64."""
    t = {}
    _, tsc = oracle.beam_search(w, cfg, raw, ev, W, L, dtype=np.float32, taps=t)
    S, nB = t["step_ids"].shape[:2]
    err, left = _beam_errors(t["step_logits"], t["step_alignments"], t["step_ids"], t["parent_ids"], np.full(nB, S), tsc, o, osc)
    _stays(left, nB, tag)
    err.update(_memory_errors(t["enc_output"], t["keys"], o))
    return err


def _twin_greedy(oracle, w, cfg, raw, ev, L, og, olg, o, tag):
    """The same for a greedy search whose fp64 pass gave (og, olg, taps o)."""
    t = {}
    tg, tlg = oracle.greedy_search(w, cfg, raw, ev, L, dtype=np.float32, taps=t)
    err, left = _greedy_errors(tg, tlg, t["step_alignments"], og, olg, o)
    _stays(left, tg.shape[0], tag)
    err.update(_memory_errors(t["enc_output"], t["keys"], o))
    return err


def _assert_twin(err, twin, tag):
    """Every tensor of err (the GPU's {tensor: max |x - fp64|}) no further from fp64 than TWIN_K x the numpy fp32 twin's error on
    the same tensor + TWIN_C.  Prints one line per case -- tensor, GPU error, twin error, ratio -- before it asserts."""
    print(f"twin-relative [{tag}]: " + "; ".join(f"{k} {e:.2e} / {twin[k]:.2e} = {e / max(twin[k], 1e-300):.2f}x" for k, e in err.items()))
    for k, e in err.items():
        assert e <= TWIN_K * twin[k] + TWIN_C, (tag, k, "further from fp64 than an fp32 evaluation is", e, twin[k])


@pytest.mark.parametrize("mode,attention,enc_depth", [
    ("joint", "luong", 2), ("raw", "luong", 2), ("event", "luong", 2),
    ("joint", "bahdanau", 2), ("joint", "luong", 1), ("joint", "luong", 3)])
def test_greedy_tensors_and_strings(rv, oracle, mode, attention, enc_depth):
    bc, w = _mk(rv, mode, attention, enc_depth)
    bc.set_option("debug_taps", 1)
    raw, ev, _ = rv.synthetic.make_slab(5, 60, 12, seed=3)
    L = 14
    tok, logits = bc.greedy_search_prediction(_inputs(rv, mode, raw, ev), L)
    taps = {}
    otok, ologits = oracle.greedy_search(w, bc.cfg.oracle_cfg(), raw, ev, L, dtype=np.float64, taps=taps)
    S = otok.shape[1]
    assert tok.shape == (5, S) and logits.shape == (5, S, 7)
    B, Tm = taps["mask"].shape
    enc = bc.get_tensor("enc_output").reshape(B, Tm, 256)
    assert np.abs(enc - taps["enc_output"]).max() < TOL
    assert (bc.get_tensor("mask").reshape(B, Tm) == taps["mask"]).all()
    assert np.abs(bc.get_tensor("keys").reshape(B, Tm, 128) - taps["keys"]).max() < TOL
    al = bc.get_tensor("step_alignments").reshape(S, B, 1, Tm)[:, :, 0]
    assert np.abs(al - taps["step_alignments"]).max() < TOL
    assert np.abs(logits.numpy() - ologits).max() < TOL
    assert (tok.numpy() == otok).all()                      # beam=1 strings bit-exact
    assert bc.tokens_to_nuc_sequences(tok) == oracle.tokens_to_nuc_sequences(otok)
    tag = f"greedy per-step {mode} {attention} enc_depth {enc_depth}"
    err, _ = _greedy_errors(tok.numpy(), logits.numpy(), al, otok, ologits, taps)
    err.update(_memory_errors(enc, bc.get_tensor("keys").reshape(B, Tm, 128), taps))
    _assert_twin(err, _twin_greedy(oracle, w, bc.cfg.oracle_cfg(), raw, ev, L, otok, ologits, taps, tag), tag)
    bc.close()


@pytest.mark.parametrize("B,Tr,Te,L,dec_depth,end_bias", [(9, 120, 20, 30, 1, 0.0), (300, 50, 10, 20, 1, 1.2), (7, 300, 30, 24, 2, 0.8),
                                                          (1, 33, 0, 12, 1, 2.0)])
def test_persistent_greedy_matches_per_step_and_oracle(rv, oracle, B, Tr, Te, L, dec_depth, end_bias):
    """greedy_search_prediction on the one-launch decode: rows keep sampling after their own end token and the slab stops
    at the step where the LAST row finishes (chunks report their first finished step through two global counters)."""
    mode = "joint" if Te else "raw"
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, decoder_depth=dec_depth, max_batch=B)
    flat = rv.weights.init_weights(bc.cfg, seed=17)
    flat["b_fc"][bc.cfg.end_token] = end_bias            # rows finish at different steps (or never)
    bc.set_weights_flat(flat)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(B, Tr, max(Te, 1), seed=B)
    x = (raw, ev) if mode == "joint" else raw
    out = {}
    bc.set_option("profile", 1)
    for persist in (1, 0):
        bc.set_option("persistent_decode", persist)
        bc.set_option("persist_taps", persist)
        bc.reset_profile()
        tok, lg = bc.greedy_search_prediction(x, L)
        assert ("dec_persist" in bc.profile()) == bool(persist)
        out[persist] = (tok.numpy().copy(), lg.numpy().copy())
        if persist:
            al = bc.get_tensor("step_alignments").reshape(tok.shape[1], B, 1, -1)[:, :min(B, 12)].copy()
    assert out[1][0].shape == out[0][0].shape and (out[1][0] == out[0][0]).all()
    assert np.abs(out[1][1] - out[0][1]).max() < TOL
    nb = min(B, 12)
    taps = {}
    ot, olg = oracle.greedy_search(w, bc.cfg.oracle_cfg(), raw[:nb], ev[:nb] if mode == "joint" else None, L, taps=taps)
    S = min(ot.shape[1], out[1][0].shape[1])              # the oracle's sub-slab may stop earlier than the full slab
    assert (out[1][0][:nb, :S] == ot[:, :S]).all() and np.abs(out[1][1][:nb, :S] - olg[:, :S]).max() < TOL
    # alignments of every step both ran (a greedy chunk runs on after its own first finished step, cs[b]: the slab's last step)
    worst = _check_alignments(al, taps["step_alignments"][:, :, None], taps["mask"], np.full(nb, S), f"greedy D={dec_depth}")
    print(f"greedy B={B} T_m={Tr + Te} D={dec_depth}: max |alpha - fp64| {worst:.2e}")
    bc.close()


@pytest.mark.parametrize("W", [1, 3, 5, 8])
def test_beam_search_matches_oracle(rv, oracle, W):
    bc, w = _mk(rv)
    bc.set_option("debug_taps", 1)
    raw, ev, _ = rv.synthetic.make_slab(6, 50, 10, seed=W)
    L = 16
    tok, sc = bc.beam_search_prediction((raw, ev), beam_width=W, max_output_len=L)
    taps = {}
    otok, osc = oracle.beam_search(w, bc.cfg.oracle_cfg(), raw, ev, W, L, dtype=np.float64, taps=taps)
    assert tok.shape == otok.shape
    S = otok.shape[1]
    lg = bc.get_tensor("step_logits").reshape(S, 6, W, 7)
    # logits of live beams (dead -inf beams at step 0 carry identical state in both)
    assert np.abs(lg - taps["step_logits"]).max() < TOL
    assert (bc.get_tensor("step_ids").reshape(S, 6, W) == taps["step_ids"]).all()
    assert (bc.get_tensor("parent_ids").reshape(S, 6, W) == taps["parent_ids"]).all()
    assert (tok.numpy() == otok).all()
    assert np.abs(sc.numpy() - osc).max() < TOL
    bc.close()


@pytest.mark.parametrize("B,Tr,Te", [(3, 40, 9), (130, 300, 30), (257, 100, 11)])
def test_memory_projection_split_gemm_against_fp64(rv, B, Tr, Te):
    """The attention-memory projection enc_output . [W_mem | A_c] (tap "projected_memory") on split-f16 MFMAs (default) and on f32 MFMAs
    (split_projection = 0), each against the fp64 product of the tapped enc_output with the weights: the split form is no further
    from fp64 than the f32 MFMA GEMM (x 1.5 + 1e-6), row counts that are not multiples of the 128-row tile included."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=B, max_raw_len=Tr, max_event_len=Te)
    flat = rv.weights.init_weights(bc.cfg, seed=9, gain=2.0)
    flat["W_mem"][:, 5] *= 25.0; flat["W_att"][128 + 7, 3] = 6.0      # a large key column, an outlier in A_c
    bc.set_weights_flat(flat)
    raw, ev, _ = rv.synthetic.make_slab(B, Tr, Te, seed=B, max_raw_pad=min(15, Tr - 1), max_event_pad=min(10, Te - 1))
    wmp = np.concatenate([flat["W_mem"], flat["W_att"][128:384]], axis=1).astype(np.float64)       # [256, 256]
    err = {}
    for split in (2, 0):
        bc.set_option("split_projection", split)
        bc.beam_search_prediction((raw, ev), 3, 5)
        enc = bc.get_tensor("enc_output").reshape(B, -1, 256).astype(np.float64)
        got = bc.get_tensor("projected_memory").reshape(B, -1, 256)
        err[split] = float(np.abs(got - enc @ wmp).max())
    print("max |projected_memory - fp64|:", err)
    assert err[0] < 1e-4 and err[2] <= 1.5 * err[0] + 1e-6, err
    bc.close()


@pytest.mark.parametrize("W,Tr,Te", [(2, 40, 9), (5, 200, 30), (7, 300, 45), (5, 300, 45), (1, 17, 3)])
def test_matrix_attention_matches_fp32_rows_and_oracle(rv, oracle, W, Tr, Te):
    """rv_set_option("matrix_attention") / ("matrix_cell"): scores and context of the persistent decode as split-f16 MFMAs on fragments
    resident in registers, and the decoder cell's product on streamed split-f16 fragments (both on: the default), against packed fp32 FMAs
    on fp32 rows: every step's logits within 2e-5 of each other and within
    1e-4 of the fp64 oracle, tokens / beam ids / parents identical, at the three memory-length variants of the kernel
    (T_m <= 64, <= 256, <= 352), with padded steps at both ends of the memory and weights scaled up (larger keys)."""
    B, L = 7, 14
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=B, max_raw_len=Tr, max_event_len=Te)
    flat = rv.weights.init_weights(bc.cfg, seed=50 + W, gain=1.5)
    flat["b_fc"][bc.cfg.end_token] = 0.3
    bc.set_weights_flat(flat)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(B, Tr, Te, seed=W, max_raw_pad=min(15, Tr - 1), max_event_pad=min(10, Te - 1))
    raw[2, Tr // 3:] = 0.0                        # a chunk with most of its raw steps padded
    bc.set_option("persist_taps", 1)
    bc.set_option("profile", 1)
    got = {}
    for mx in (2, 1, 0):                          # 2: attention AND the cell product on the matrix pipe (the default), 1: attention only
        bc.set_option("matrix_attention", 1 if mx else 0)
        bc.set_option("matrix_cell", 1 if mx == 2 else 0)
        tok, sc = bc.beam_search_prediction((raw, ev), W, L)
        assert "dec_persist" in bc.profile()
        cs = bc.get_tensor("chunk_steps").astype(int)
        S = tok.shape[1]
        got[mx] = (tok.numpy().copy(), sc.numpy().copy(), cs, bc.get_tensor("step_logits").reshape(S, B, W, 7).copy(),
                   bc.get_tensor("step_ids").reshape(S, B, W).copy(), bc.get_tensor("parent_ids").reshape(S, B, W).copy(),
                   bc.get_tensor("step_alignments").reshape(S, B, W, Tr + Te).copy())
    taps = {}
    otok, osc = oracle.beam_search(w, bc.cfg.oracle_cfg(), raw, ev, W, L, dtype=np.float64, taps=taps)
    twin = _twin_beam(oracle, w, bc.cfg.oracle_cfg(), raw, ev, W, L, taps, osc, f"matrix_attention W={W} T_m={Tr + Te}")
    worst = {}
    for mx in (2, 1, 0):
        tok, sc, cs, lg, ids, par, al = got[mx]
        assert tok.shape == otok.shape and (tok == otok).all() and np.abs(sc - osc).max() < TOL, mx
        for b in range(B):
            n = cs[b]
            assert np.abs(lg[:n, b] - taps["step_logits"][:n, b]).max() < TOL, (mx, b)
            assert (ids[:n, b] == taps["step_ids"][:n, b]).all() and (par[:n, b] == taps["parent_ids"][:n, b]).all(), (mx, b)
        # alignments: the f16 hi / lo image the context product consumes (mx 2, 1), the fp32 rows (mx 0)
        worst[mx] = _check_alignments(al, taps["step_alignments"], taps["mask"], cs, f"matrix_attention form {mx}")
        _assert_twin(_beam_errors(lg, al, ids, par, cs, sc, taps, osc)[0], twin, f"matrix_attention W={W} T_m={Tr + Te} form {mx}")
    print(f"W={W} T_m={Tr + Te}: max |alpha - fp64| by form (2: ATT 3, 1: ATT 2, 0: ATT 0):", worst)
    assert (got[1][2] == got[0][2]).all() and (got[2][2] == got[0][2]).all()
    for b in range(B):
        n = got[1][2][b]
        assert np.abs(got[1][3][:n, b] - got[0][3][:n, b]).max() < 2e-5, b
        assert np.abs(got[2][3][:n, b] - got[0][3][:n, b]).max() < 2e-5, b
        assert np.abs(got[1][6][:n, b] - got[0][6][:n, b]).max() < 2e-5, b
        assert np.abs(got[2][6][:n, b] - got[0][6][:n, b]).max() < 2e-5, b
    bc.close()


@pytest.mark.parametrize("W,dec_depth", [(1, 1), (5, 1), (8, 1), (3, 2)])
def test_persistent_decode_step_logits(rv, oracle, W, dec_depth):
    """Tensor-level check of the DEFAULT product path in beam mode: the one-launch persistent decode records its
    per-step logits (option persist_taps); logits <= 1e-4, ids / parents identical to the fp64 oracle, for every
    step a chunk ran (a chunk stops recording at its own last step, `chunk_steps`)."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, decoder_depth=dec_depth, max_batch=16)
    flat = rv.weights.init_weights(bc.cfg, seed=13)
    flat["b_fc"][bc.cfg.end_token] = 0.5          # chunks stop at different steps
    bc.set_weights_flat(flat)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    B, L = 9, 18
    raw, ev, _ = rv.synthetic.make_slab(B, 70, 14, seed=40 + W)
    bc.set_option("persist_taps", 1)
    bc.set_option("profile", 1)
    taps = {}
    otok, osc = oracle.beam_search(w, bc.cfg.oracle_cfg(), raw, ev, W, L, dtype=np.float64, taps=taps)
    S = otok.shape[1]
    twin = _twin_beam(oracle, w, bc.cfg.oracle_cfg(), raw, ev, W, L, taps, osc, f"persistent W={W} D={dec_depth}")
    # the default form (all on the matrix pipe: ATT 3); with two cells also both cells on packed FMAs (ATT 0, matrix_cell = 0)
    for mcell in ((1, 0) if dec_depth == 2 else (1,)):
        bc.set_option("matrix_cell", mcell)
        bc.reset_profile()
        tok, sc = bc.beam_search_prediction((raw, ev), W, L)
        assert "dec_persist" in bc.profile()                     # the persistent kernel ran, not the per-step path
        assert tok.shape == otok.shape and (tok.numpy() == otok).all() and np.abs(sc.numpy() - osc).max() < TOL
        cs = bc.get_tensor("chunk_steps").astype(int)
        assert cs.max() == S and (cs >= 1).all()
        lg = bc.get_tensor("step_logits").reshape(S, B, W, 7)
        ids = bc.get_tensor("step_ids").reshape(S, B, W)
        par = bc.get_tensor("parent_ids").reshape(S, B, W)
        for b in range(B):
            n = cs[b]
            assert np.abs(lg[:n, b] - taps["step_logits"][:n, b]).max() < TOL, b
            assert (ids[:n, b] == taps["step_ids"][:n, b]).all() and (par[:n, b] == taps["parent_ids"][:n, b]).all(), b
        al = bc.get_tensor("step_alignments").reshape(S, B, W, 84)
        worst = _check_alignments(al, taps["step_alignments"], taps["mask"], cs, f"W={W} D={dec_depth} matrix_cell={mcell}")
        print(f"W={W} D={dec_depth} matrix_cell={mcell}: max |alpha - fp64| {worst:.2e}")
        _assert_twin(_beam_errors(lg, al, ids, par, cs, sc.numpy(), taps, osc)[0], twin, f"persistent W={W} D={dec_depth} matrix_cell={mcell}")
    bc.close()


# ----------------------------------------------------------------------------------------------
# committed golden fixtures (tests/golden, regenerated by make_golden.py from exact seeds)
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden_mod():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("name", ["joint_luong_w5", "joint_bahdanau_w3", "raw_luong_greedy", "event_luong_w2_d1"])
def test_golden_fixtures_on_gpu(rv, name):
    mg = _golden_mod()
    cfg, flat, w, raw, ev, W, L = mg.build(name)
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, cfg.mode, 0.0, encoder_depth=cfg.enc_depth,
                       attention_type=cfg.attention, honor_attention_type=True, max_batch=8)
    bc.set_weights_flat(flat)
    bc.set_option("debug_taps", 1)
    inp = _inputs(rv, cfg.mode, raw, ev)
    if "greedy" in name:
        tok, logits = bc.greedy_search_prediction(inp, L)
        assert np.abs(logits.numpy() - g["logits"]).max() < TOL
    else:
        tok, sc = bc.beam_search_prediction(inp, W, L)
        assert np.abs(sc.numpy() - g["scores"]).max() < TOL
        S = g["tokens"].shape[1]
        assert (bc.get_tensor("step_ids").reshape(S, -1, W) == g["step_ids"]).all()
        assert np.abs(bc.get_tensor("step_logits").reshape(g["step_logits"].shape) - g["step_logits"]).max() < TOL
    assert (tok.numpy() == g["tokens"]).all()
    assert bc.tokens_to_nuc_sequences(tok) == [str(x) for x in g["strings"]]
    B, Tm = g["mask"].shape
    assert (bc.get_tensor("mask").reshape(B, Tm) == g["mask"]).all()
    assert np.abs(bc.get_tensor("enc_output").reshape(B, Tm, 256)[:, ::5, ::16] - g["enc_output_sample"]).max() < TOL
    bc.close()


def _near_tie_gap(oracle, lg, W, end):
    """Replay the fp64 beam steps of ONE chunk from its step logits lg [S, W, V]: the smallest gap between two neighbours among the
    W + 1 best candidates of any step (a gap below fp32 resolution can legitimately be ordered either way)."""
    log_probs = np.full((1, W), -np.inf); log_probs[0, 0] = 0.0
    fin = np.zeros((1, W), bool); ln = np.zeros((1, W), np.int64)
    gap = np.inf
    for s_ in range(lg.shape[0]):
        lp = oracle.log_softmax(lg[s_][None])
        row = np.full((lg.shape[2],), oracle.F32_MIN); row[end] = 0.0
        lp = np.where(fin[..., None], row, lp)
        total = np.sort((log_probs[..., None] + lp).reshape(-1))[::-1]
        top = total[:W + 1]
        top = top[np.isfinite(top)]
        if top.size > 1:
            gap = min(gap, float(np.min(-np.diff(top))))
        _, _, _, log_probs, fin, ln = oracle.beam_search_step(lg[s_][None], log_probs, fin, ln, end)
    return gap


def _score_tol(sc):
    """Tolerance for CUMULATIVE beam scores: the per-step tolerance plus what fp32 accumulation itself may lose -- the reference adds
    one log-probability per step to a running fp32 sum, each addition rounding by up to half an ulp of the sum
    (|score| ~ 100 after 63 steps of peaky weights: 63 x 3.8e-6)."""
    sc = np.asarray(sc, np.float32)
    if sc.size == 0:
        return TOL
    return TOL + 0.5 * sc.shape[-1] * float(np.spacing(np.float32(np.abs(sc).max())))


def _explain_mismatches(rv, oracle, bc, flat, mode, raw, ev, W, L, tok, ctok, tag="", sc=None, csc=None):
    """Rows on which the GPU and the fp32 C port disagree -- in their tokens, or (tokens equal) in the per-step top-1 scores by
    1e-4 or more -- are not waved through: each one is re-decoded ALONE by the fp64 numpy oracle.  Accepted: the GPU's tokens and
    scores equal the fp64 ones (the C port is the one that flipped), or the fp64 decode of that chunk passes through a near-tie --
    two of its W + 1 best candidates of some step closer than 1e-4 -- which fp32 rounding can legitimately resolve either way
    (a different beam set after the cut also changes the later top-1 scores, which are not back-traced: SURVEY.md A.5).
    Anything else fails and prints the row.  Returns the mask of rows that agree outright and the number that needed explaining."""
    same = (tok == ctok).all(axis=1)
    stol = _score_tol(sc) if sc is not None else TOL
    if sc is not None:
        same &= np.abs(sc - csc).max(axis=1, initial=0.0) < stol
    bad = np.nonzero(~same)[0]
    assert same.mean() >= 0.95, f"{tag}: only {100 * same.mean():.2f} % rows identical"
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    cfg = bc.cfg.oracle_cfg()
    end = cfg["end_token"]
    unexplained = []
    for b in bad:
        r1 = raw[b:b + 1] if mode != "event" else None
        e1 = ev[b:b + 1] if mode != "raw" else None
        taps = {}
        otok, osc = oracle.beam_search(w, cfg, r1, e1, W, L, dtype=np.float64, taps=taps)
        S = otok.shape[1]
        got = tok[b, :S]
        if got.shape[0] == S and (got == otok[0]).all() and (tok[b, S:] == end).all() and \
                (sc is None or np.abs(sc[b, :S] - osc[0]).max(initial=0.0) < stol):
            continue                                       # GPU == fp64: the C port took the other side of a tie
        gap = _near_tie_gap(oracle, taps["step_logits"][:, 0], W, end)
        if gap < TOL:
            continue                                       # a genuine near-tie in the exact arithmetic
        unexplained.append((int(b), gap, got.tolist(), otok[0].tolist()))
    assert not unexplained, f"{tag}: rows that differ from fp64 with no near-tie: {unexplained[:3]}"
    return same, len(bad)


# ----------------------------------------------------------------------------------------------
# BASELINE.json full sizes against the C port of the oracle (numpy is too slow there)
def _emitting_flat(rv, cfg, seed=22, end_bias=-1.0):
    """Random weights biased to call bases (gain 3, base letters + 1.5, end token lowered): at Keras-default weights nearly every
    best hypothesis at BASELINE sizes is a row of end tokens, and "tokens identical" is then nearly free."""
    flat = rv.weights.init_weights(cfg, seed=seed, gain=3.0)
    letters = [t for t in range(cfg.vocab) if t not in (cfg.start_token, cfg.end_token, cfg.pad_token)]   # a c g t = 3..6 of nuc_tk
    flat["b_fc"][letters] += 1.5
    flat["b_fc"][cfg.end_token] += end_bias
    return flat


def _assert_calls_are_strings(rv, bc, tok, tag):
    """The compared rows are non-trivial: most best hypotheses hold several base letters and the calls differ between chunks."""
    seqs = bc.tokens_to_nuc_sequences(tok)
    lens = np.array([len(s) for s in seqs])
    assert np.median(lens) >= 5 and len(set(seqs)) > 0.2 * len(seqs), (tag, np.median(lens), len(set(seqs)))
    return lens


@pytest.mark.parametrize("weights", ["keras", "emitting"])
@pytest.mark.parametrize("B,T_r,T_e,W,L,tag", [
    (64, 300, 30, 1, 48, "C2"), (256, 300, 30, 5, 48, "C3"), (1024, 200, 30, 5, 32, "R"), (67, 123, 17, 4, 20, "ragged")])
def test_full_size_against_c_port(rv, oracle, B, T_r, T_e, W, L, tag, weights):
    from oracle import cpu_port
    bc, _ = _mk(rv, max_batch=B, max_raw_len=T_r, max_event_len=T_e, max_output_len=L)
    flat = rv.weights.init_weights(bc.cfg, seed=22) if weights == "keras" else _emitting_flat(rv, bc.cfg)
    bc.set_weights_flat(flat)
    raw, ev, _ = rv.synthetic.make_slab(B, T_r, T_e, seed=17)
    tok, sc = bc.beam_search_prediction((raw, ev), W, L)
    ctok, csc = cpu_port.run(bc.cfg.oracle_cfg(), 2, 7, rv.weights.pack(bc.cfg, flat), raw, ev, W, L)
    assert tok.shape == ctok.shape, tag
    tag = f"{tag}/{weights}"
    if weights == "emitting":
        lens = _assert_calls_are_strings(rv, bc, tok, tag)
        print(f"{tag}: call lengths min / median / max {lens.min()} / {int(np.median(lens))} / {lens.max()}, {len(set(bc.tokens_to_nuc_sequences(tok)))} distinct calls")
    # fp32-vs-fp32 at 10^5 candidates: every row that differs must be explained by the fp64 oracle (100 % rows accounted for)
    same, n_bad = _explain_mismatches(rv, oracle, bc, flat, "joint", raw, ev, W, L, tok.numpy(), ctok, tag, sc.numpy(), csc)
    print(f"{tag}: {n_bad} of {B} rows differ from the C port (tokens, or scores by >= 1e-4), all explained by the fp64 oracle")
    # size-independent properties: scores non-increasing, per-base probabilities in (0, 1]
    s = sc.numpy()
    assert (np.diff(s, axis=1) <= 1e-6).all()
    p = rv.utils.calc_prob_logits_beam_search_scores(sc).numpy()
    assert (p > 0).all() and (p <= 1 + 1e-6).all()
    # idempotence / determinism: a second call returns the same bytes
    tok2, sc2 = bc.beam_search_prediction((raw, ev), W, L)
    assert (tok2.numpy() == tok.numpy()).all() and np.array_equal(sc2.numpy(), sc.numpy())
    bc.close()


def test_flash_and_two_pass_attend_agree(rv, oracle):
    bc, w = _mk(rv)
    raw, ev, _ = rv.synthetic.make_slab(16, 90, 20, seed=8)
    out = {}
    for flash, nt in ((1, 512), (0, 0), (2, 256)):          # 2 = single-pass, 256-thread variant
        bc.set_option("flash_attend", 1 if flash else 0)
        bc.set_option("attend_threads", nt)
        bc.set_option("debug_taps", 1)
        tok, sc = bc.beam_search_prediction((raw, ev), 5, 20)
        out[flash] = (tok.numpy().copy(), sc.numpy().copy(), bc.get_tensor("step_alignments"), bc.get_tensor("step_logits"))
    for other in (1, 2):
        assert (out[0][0] == out[other][0]).all()
        assert np.abs(out[0][1] - out[other][1]).max() < TOL
        assert np.abs(out[0][2] - out[other][2]).max() < TOL and np.abs(out[0][3] - out[other][3]).max() < TOL
    taps = {}
    oracle.beam_search(w, bc.cfg.oracle_cfg(), raw[:4], ev[:4], 5, 20, taps=taps)
    S = taps["step_alignments"].shape[0]
    al = out[1][2].reshape(out[1][0].shape[1], 16, 5, -1)[:S, :4]
    assert np.abs(al - taps["step_alignments"]).max() < TOL
    bc.close()


@pytest.mark.parametrize("B,Tr,Te,W,L,dec_depth", [(16, 90, 20, 5, 20, 1), (9, 300, 30, 5, 32, 1), (5, 40, 8, 3, 12, 1),
                                                   (7, 200, 0, 1, 16, 1), (6, 0, 45, 4, 14, 1), (3, 320, 32, 2, 10, 1),
                                                   (11, 120, 25, 5, 24, 2), (4, 300, 30, 3, 12, 2), (6, 60, 0, 1, 10, 2),
                                                   (10, 300, 30, 8, 20, 1), (5, 100, 12, 6, 16, 1), (3, 30, 45, 7, 12, 1)])
def test_persistent_decode_matches_per_step_graph(rv, oracle, B, Tr, Te, W, L, dec_depth):
    """One-launch register-resident decode == per-step kernels == oracle (tokens exact, scores within TOL); one and two
    stacked decoder cells (the reference's decd1 / decd2 model families)."""
    mode = "joint" if Tr and Te else ("raw" if Tr else "event")
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, decoder_depth=dec_depth, max_batch=32, max_raw_len=320)
    flat = rv.weights.init_weights(bc.cfg, seed=11)
    flat["b_fc"][bc.cfg.end_token] = 0.6          # chunks finish at different steps
    bc.set_weights_flat(flat)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(B, max(Tr, 1), max(Te, 1), seed=B)
    raw[1, Tr // 2:] = 0.0                        # a chunk with trailing padding (masked steps)
    x = (raw, ev) if mode == "joint" else (raw if mode == "raw" else ev)
    out = {}
    bc.set_option("profile", 1)
    for persist in (1, 0):
        bc.set_option("persistent_decode", persist)
        bc.reset_profile()
        tok, sc = bc.beam_search_prediction(x, W, L)
        out[persist] = (tok.numpy().copy(), sc.numpy().copy())
        assert ("dec_persist" in bc.profile()) == bool(persist)
    assert out[1][0].shape == out[0][0].shape and (out[1][0] == out[0][0]).all()
    assert np.abs(out[1][1] - out[0][1]).max() < TOL
    ot, osc = oracle.beam_search(w, bc.cfg.oracle_cfg(), raw if mode != "event" else None, ev if mode != "raw" else None, W, L)
    assert out[1][0].shape == ot.shape and (out[1][0] == ot).all() and np.abs(out[1][1] - osc).max() < TOL
    bc.close()


@pytest.mark.parametrize("mode,B,Tr,Te,depth", [("joint", 5, 37, 9, 2), ("raw", 3, 7, 1, 2), ("event", 130, 1, 45, 3),
                                               ("joint", 300, 100, 30, 2), ("raw", 1, 300, 1, 4), ("joint", 600, 24, 5, 2)])
def test_fused_projection_matches_gemm_path_and_oracle(rv, oracle, mode, B, Tr, Te, depth):
    """Encoder layers >= 1 with the input projection on MFMA waves inside the recurrence kernel == the separate GEMM
    launch (fp32, different summation order: <= 1e-5) == the oracle (<= TOL); block sizes 16/BT with ragged T."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=depth, max_batch=B)
    flat = bc.init_random_weights(seed=7)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(B, Tr, Te, seed=depth, max_raw_pad=min(15, Tr - 1), max_event_pad=min(10, Te - 1))
    x = _inputs(rv, mode, raw, ev)
    enc = {}
    bc.set_option("wide_recurrence", 0)                    # this test is about the packed-FMA kernels and their fused projection
    for fuse in (1, 0):
        bc.set_option("fused_projection", fuse)
        tok, sc = bc.beam_search_prediction(x, 3, 6)
        enc[fuse] = (bc.get_tensor("enc_output").copy(), tok.numpy().copy())
    assert np.abs(enc[1][0] - enc[0][0]).max() < 1e-5 and (enc[1][1] == enc[0][1]).all()
    nb = min(B, 6)
    r_, e_ = raw[:nb] if mode != "event" else None, ev[:nb] if mode != "raw" else None
    o_enc, _ = oracle.encode_input(w, r_, e_, mode)
    t_enc, _ = oracle.encode_input(w, r_, e_, mode, 0.0, np.float32)
    twin = dict(enc_output=float(np.abs(t_enc - o_enc).max()))
    got = enc[1][0].reshape(B, -1, 256)[:nb]
    assert np.abs(got - o_enc).max() < TOL
    for fuse in (1, 0):
        got = enc[fuse][0].reshape(B, -1, 256)[:nb]
        _assert_twin(dict(enc_output=float(np.abs(got - o_enc).max())), twin, f"packed FMA {mode} B={B} depth={depth} fused_projection={fuse}")
    bc.close()


@pytest.mark.parametrize("mode,B,Tr,Te,depth", [("joint", 5, 37, 9, 2), ("raw", 3, 7, 1, 2), ("event", 130, 1, 45, 3), ("joint", 33, 300, 30, 2),
                                                 ("joint", 16, 64, 12, 1), ("joint", 600, 200, 30, 2)])
def test_matrix_pipe_recurrence_matches_fma_path_and_oracle(rv, oracle, mode, B, Tr, Te, depth):
    """`wide_recurrence` (lstm_mx.hip): the encoder recurrences as one split-f16 MFMA product per step for 16 chunks of a
    direction per workgroup, raw layer 0 with its input projection in the lane, event layer 0 / layers >= 1 on pre-projected inputs
    (elementwise kernel / split-f16 GEMM over both directions) -- against the packed-FMA kernels of the same library and the fp64
    oracle: enc_output within 1e-4 of the oracle and as close to it as the FMA path (x 2 + 1e-6), slabs that are not multiples of
    16 chunks, one to three layers (state chaining), all three input modes; beam-search tokens identical, scores within 1e-4."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=depth, max_batch=B, max_raw_len=max(Tr, 1),
                       max_event_len=max(Te, 1))
    flat = bc.init_random_weights(seed=11 + depth, gain=2.0)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(B, Tr, Te, seed=B, max_raw_pad=min(15, Tr - 1), max_event_pad=min(10, Te - 1))
    x = _inputs(rv, mode, raw, ev)
    out, enc = {}, {}
    bc.set_option("profile", 1)
    for wide in (1, 2, 0):                                  # 16 chunks per workgroup; 8 (the latency form: both f16 parts of h in the product's columns); packed FMA
        bc.set_option("wide_recurrence", wide)
        bc.reset_profile()
        tok, sc = bc.beam_search_prediction(x, 5, 12)
        names = set(bc.profile())
        assert (("gemm_inproj_raw" in names or "gemm_inproj_event" in names) == bool(wide)) or depth == 1
        out[wide] = (tok.numpy().copy(), sc.numpy().copy())
        enc[wide] = bc.get_tensor("enc_output").reshape(B, -1, 256)
    nb = min(B, 24)
    r_, e_ = raw[:nb] if mode != "event" else None, ev[:nb] if mode != "raw" else None
    e64, _ = oracle.encode_input(w, r_, e_, mode, 0.0, np.float64)
    e32, _ = oracle.encode_input(w, r_, e_, mode, 0.0, np.float32)
    twin = dict(enc_output=float(np.abs(e32 - e64).max()))
    err = {k: float(np.abs(enc[k][:nb] - e64).max()) for k in enc}
    print(f"{mode} B={B} depth={depth}: max |enc_output - fp64| matrix pipe {err[1]:.2e}, its 8-chunk form {err[2]:.2e}, packed FMA {err[0]:.2e}")
    for k in (1, 2, 0):
        _assert_twin(dict(enc_output=err[k]), twin, f"recurrence {mode} B={B} depth={depth} wide_recurrence={k}")
    for k in (1, 2):
        assert err[k] < TOL and err[k] <= 2.0 * err[0] + 1e-6, err
        assert np.abs(enc[k] - enc[0]).max() < TOL
        assert out[k][0].shape == out[0][0].shape and np.abs(out[k][1] - out[0][1]).max() < TOL
        same = (out[k][0] == out[0][0]).all(axis=1)
        assert same.mean() >= 0.98, same.mean()             # (a near-tie may flip between two fp32 paths; test_full_size explains such rows)
    bc.close()


@pytest.mark.parametrize("mode,B,Tr,Te,wide", [("joint", 37, 60, 17, 1), ("event", 130, 1, 45, 1), ("joint", 21, 40, 30, 2), ("event", 9, 1, 1, 2)])
def test_event_projection_in_the_lane_is_bit_identical(rv, mode, B, Tr, Te, wide):
    """Option lane_projection: the event encoder's layer 0 with its five-feature input projection inside the matrix-pipe recurrence (inputs
    staged in LDS, the same fused multiply-adds in the same order) against k_inproj_small + pre-projected inputs: byte-identical encoder
    output, input mask, tokens and scores; padded events (the mask's all-features test), slabs that are not multiples of 8 / 16 chunks, both
    workgroup sizes of the recurrence; and the projection launch really is gone."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=2, max_batch=B, max_raw_len=max(Tr, 1), max_event_len=max(Te, 1))
    bc.init_random_weights(seed=5, gain=2.0)
    raw, ev, _ = rv.synthetic.make_slab(B, Tr, Te, seed=B, max_raw_pad=min(15, Tr - 1), max_event_pad=min(10, Te - 1))
    x = _inputs(rv, mode, raw, ev)
    bc.set_option("wide_recurrence", wide)
    bc.set_option("profile", 1)
    got = {}
    for lane in (1, 0):
        bc.set_option("lane_projection", lane)
        bc.reset_profile()
        tok, sc = bc.beam_search_prediction(x, 5, 10)
        assert ("inproj_event_l0" in bc.profile()) == (lane == 0)
        got[lane] = (tok.numpy().copy(), sc.numpy().copy(), bc.get_tensor("enc_output").copy(), bc.get_tensor("mask").copy())
    for a, b in zip(got[1], got[0]):
        assert a.shape == b.shape and np.array_equal(a, b)
    bc.close()


@pytest.mark.parametrize("scale_cols", [False, True])
def test_split_projection_is_as_close_to_fp64_as_the_f32_mfma(rv, oracle, scale_cols):
    """rv_set_option("split_projection"): the input projection of encoder layers >= 1 on 16-bit MFMAs with split operands
    (2 = two f16 parts of the scaled operands, 1 = three bf16 parts) against the f32 MFMA (0), each measured against the
    fp64 oracle's encoder output.  The split forms must be no further from fp64 than the f32 form is (x 1.5 + 2e-7 for the
    scatter of a maximum), also when some columns of the kernel are 20x larger, some 1000x smaller and one weight of a small column is an
    outlier (the per-column scaling of form 2), and every form gives the same tokens."""
    B, Tr, Te = 6, 120, 20
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=3, max_batch=B)
    flat = rv.weights.init_weights(bc.cfg, seed=31)
    if scale_cols:
        for name, a in flat.items():
            if name.startswith("enc_") and name.endswith(".W") and a.shape == (256, 512):
                a[:, 40:48] *= 20.0; a[:, 300:304] *= 1e-3; a[17, 100] = 3.0
    bc.set_weights_flat(flat)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(B, Tr, Te, seed=4, max_raw_pad=10, max_event_pad=5)
    ref, _ = oracle.encode_input(w, raw, ev, "joint")
    err, toks = {}, {}
    bc.set_option("wide_recurrence", 0)                    # the three forms of the FUSED projection (the matrix-pipe recurrence has its own test)
    for split in (0, 1, 2):
        bc.set_option("split_projection", split)
        tok, _ = bc.beam_search_prediction((raw, ev), 3, 6)
        err[split] = float(np.abs(bc.get_tensor("enc_output").reshape(ref.shape) - ref).max())
        toks[split] = tok.numpy().copy()
    print("max |enc_output - fp64|:", err)
    assert err[0] < 2e-5, err
    for split in (1, 2):
        assert err[split] <= 1.5 * err[0] + 2e-7, err
        assert (toks[split] == toks[0]).all()
    bc.close()


def test_every_documented_option_is_accepted(rv):
    """rv_set_option: every key the header documents exists, an unknown key is an error (include/ravvent_hip.h)."""
    import re
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ravvent_hip.h")).read()
    doc = hdr[hdr.index("/* Options."):hdr.index("int rv_set_option")]
    keys = set(re.findall(r'"([a-z_]+)"\s*\(', doc))
    assert {"debug_taps", "use_graph", "decode_split", "attend_threads", "flash_attend", "concurrent_encoders",
            "fused_projection", "persistent_decode", "persist_taps", "tail_wave", "split_projection", "matrix_attention", "matrix_cell", "profile",
            "wide_recurrence", "async_depth", "slab_graph", "lane_projection"} <= keys
    bc, _ = _mk(rv)
    for k in sorted(keys):
        bc.set_option(k, 1 if k != "attend_threads" else 256)
    with pytest.raises(rv._capi.RavventHipError):
        bc.set_option("no_such_option", 1)
    bc.close()


def test_device_and_host_inputs_agree(rv):
    import torch
    bc, _ = _mk(rv)
    raw, ev, _ = rv.synthetic.make_slab(8, 64, 12, seed=2)
    t1, s1 = bc.beam_search_prediction((raw, ev), 5, 12)
    t2, s2 = bc.beam_search_prediction((torch.from_numpy(raw).cuda(), torch.from_numpy(ev).cuda()), 5,
                                       torch.tensor(12))           # 0-d tensor like tf.shape(target)[1]
    assert t2.is_cuda and (t1.numpy() == t2.cpu().numpy()).all() and np.array_equal(s1.numpy(), s2.cpu().numpy())
    for use_graph in (0, 1):
        bc.set_option("use_graph", use_graph)
        t3, s3 = bc.beam_search_prediction((raw, ev), 5, 12)
        assert (t3.numpy() == t1.numpy()).all() and np.array_equal(s3.numpy(), s1.numpy())
    bc.close()


def test_edge_cases(rv, oracle):
    bc, w = _mk(rv)
    raw, ev, _ = rv.synthetic.make_slab(3, 20, 5, seed=1)
    # empty slab, and max_output_len 1 (zero decode steps)
    t, s = bc.beam_search_prediction((raw[:0], ev[:0]), 5, 10)
    assert t.shape == (0, 0)
    t, s = bc.beam_search_prediction((raw, ev), 5, 1)
    assert t.shape == (3, 0) and s.shape == (3, 0)
    # single chunk, single timestep
    t, s = bc.beam_search_prediction((raw[:1, :1], ev[:1, :1]), 2, 6)
    ot, osc = oracle.beam_search(w, bc.cfg.oracle_cfg(), raw[:1, :1], ev[:1, :1], 2, 6)
    assert (t.numpy() == ot).all() and np.abs(s.numpy() - osc).max() < TOL
    # a real sample that is exactly 0.0 counts as padding in the attention mask (utils.py:32)
    raw2 = raw.copy(); raw2[0, 3, 0] = 0.0
    bc.set_option("debug_taps", 1)
    t, s = bc.beam_search_prediction((raw2, ev), 3, 8)
    taps = {}
    ot, osc = oracle.beam_search(w, bc.cfg.oracle_cfg(), raw2, ev, 3, 8, taps=taps)
    assert (t.numpy() == ot).all() and (bc.get_tensor("mask").reshape(3, -1) == taps["mask"]).all()
    assert bc.get_tensor("mask").reshape(3, -1)[0, 3] == 0
    # argument errors come back as exceptions carrying the C-ABI message
    with pytest.raises(rv._capi.RavventHipError, match="beam width"):
        bc.beam_search_prediction((raw, ev), 9, 8)
    with pytest.raises(rv._capi.RavventHipError, match="max_output_len"):
        bc.beam_search_prediction((raw, ev), 5, 1000)
    with pytest.raises(ValueError):
        bc.beam_search_prediction((raw, ev[:2]), 5, 8)
    bc.close()


def test_early_finish_stops_the_loop(rv, oracle):
    """A strong end-token bias makes every beam finish early: S < L-1, finished beams keep their
    score, gather_tree pads with the end token."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=16)
    flat = rv.weights.init_weights(bc.cfg, seed=3)
    flat["b_fc"][1] = 2.5
    bc.set_weights_flat(flat)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(12, 50, 10, seed=4)
    for W in (1, 5):
        tok, sc = bc.beam_search_prediction((raw, ev), W, 40)
        ot, osc = oracle.beam_search(w, bc.cfg.oracle_cfg(), raw, ev, W, 40)
        assert tok.shape == ot.shape and tok.shape[1] < 39
        assert (tok.numpy() == ot).all() and np.abs(sc.numpy() - osc).max() < TOL
        # chunks finish at different steps here: the finished-chunk fast path of the per-step kernels (no attention for a
        # chunk whose beams are all done) must not change a bit relative to the taps-on run, which disables it; the
        # persistent decode (a different summation order) agrees with both to f32 rounding
        bc.set_option("persistent_decode", 0)
        tok1, sc1 = bc.beam_search_prediction((raw, ev), W, 40)
        bc.set_option("debug_taps", 1)
        tok2, sc2 = bc.beam_search_prediction((raw, ev), W, 40)
        bc.set_option("debug_taps", 0); bc.set_option("persistent_decode", 1)
        assert (tok2.numpy() == tok1.numpy()).all() and np.array_equal(sc2.numpy(), sc1.numpy())
        assert (tok1.numpy() == tok.numpy()).all() and np.abs(sc1.numpy() - sc.numpy()).max() < 1e-6
    g, lg = bc.greedy_search_prediction((raw, ev), 40)
    og, olg = oracle.greedy_search(w, bc.cfg.oracle_cfg(), raw, ev, 40)
    assert g.shape == og.shape and (g.numpy() == og).all() and np.abs(lg.numpy() - olg).max() < TOL
    bc.close()


def test_evaluator_call_sequence(rv):
    bc, _ = _mk(rv, max_batch=64)
    raw, ev, nuc = rv.synthetic.make_slab(150, 60, 10, seed=6, L=14)
    res = rv.evaluator.PerformanceEvaluator(bc, fused_postprocessing=False).run_slabs(raw, ev, nuc, chunk_size=64)     # the reference's host sequence
    for key in ("bases_num", "samples_num", "t_data_loading", "t_predicting", "t_postprocessing", "t_merge",
                "total", "total_processing"):        # ravvent_performance_evaluator.py:78-87
        assert key in res
    assert res["chunks_num"] == 150 and len(res["nuc_preds"]) == 150
    seq, probs = res["nuc_preds"][0]
    assert len(seq) == len(probs) and set(seq) <= set("ACGT")
    # t_merge: the C++ merger over the same per-chunk calls == the merger oracle on them
    from oracle import merger_oracle
    assert res["t_merge"] > 0 and res["merged_seq"] == merger_oracle.merge(res["nuc_preds"])[0]
    fused = rv.evaluator.PerformanceEvaluator(bc, fused_postprocessing=True).run_slabs(raw, ev, nuc, chunk_size=64)
    assert fused["merged_seq"] == res["merged_seq"]
    piped = rv.evaluator.PerformanceEvaluator(bc, pipelined_merge=True).run_slabs(raw, ev, nuc, chunk_size=64)
    assert piped["merged_seq"] == res["merged_seq"] and [p[0] for p in piped["nuc_preds"]] == [p[0] for p in res["nuc_preds"]]
    # two handles decoding consecutive slabs at the same time from two host threads: same calls, same read
    ev2 = rv.evaluator.PerformanceEvaluator(bc, pipelined_merge=True, concurrent_slabs=2)
    conc = ev2.run_slabs(raw, ev, nuc, chunk_size=32)
    assert conc["merged_seq"] == rv.evaluator.PerformanceEvaluator(bc, pipelined_merge=True).run_slabs(raw, ev, nuc, chunk_size=32)["merged_seq"]
    assert [p[0] for p in conc["nuc_preds"]] == [p[0] for p in res["nuc_preds"]]
    ev2.close()
    bc.close()


def test_read_level_pipeline(rv):
    """signal -> events -> chunks (reference-native 200 samples + 30 events) -> slabs -> calls."""
    bc, _ = _mk(rv, max_batch=256, max_raw_len=200, max_event_len=30, max_output_len=40)
    sig, lab = rv.synthetic.make_read(1200, seed=3)
    res = rv.evaluator.PerformanceEvaluator(bc).run_read(sig, lab, chunk_size=256)
    assert res["bases_num"] == 1200 and res["chunks_num"] > 100 and res["samples_num"] == int(lab[-1, 1]) - int(lab[0, 0])
    assert len(res["nuc_preds"]) == res["chunks_num"] and res["total_processing"] > 0
    assert res["t_merge"] > 0 and set(res["merged_seq"]) <= set("ACGT")
    bc.close()


def test_many_reads_share_slabs(rv):
    """evaluator.run_many: chunks of several reads queued into common slabs == every read evaluated alone."""
    bc, _ = _mk(rv, max_batch=64)
    ev_ = rv.evaluator.PerformanceEvaluator(bc, fused_postprocessing=True)
    reads = []
    for i, n in enumerate((37, 5, 0, 90, 64)):
        raw, ev, nuc = rv.synthetic.make_slab(max(n, 1), 60, 10, seed=20 + i, L=12)
        reads.append((raw[:n], ev[:n], nuc[:n]))
    out = ev_.run_many(reads, chunk_size=64)
    assert len(out) == 5 and out[0]["timing"]["chunks_num"] == 196 and out[2]["merged_seq"] == ""
    for i, r in enumerate(reads):
        if r[0].shape[0] == 0:
            continue
        alone = ev_.run_slabs(*r, chunk_size=64)
        assert out[i]["merged_seq"] == alone["merged_seq"] and out[i]["chunks_num"] == alone["chunks_num"]
    bc.close()


def test_random_shapes_against_c_port(rv, oracle):
    """Shape fuzz: ragged batch / time / beam / length combinations in all three input modes."""
    from oracle import cpu_port
    rng = np.random.default_rng(2024)
    handles = {}
    for case in range(12):
        mode = ("joint", "raw", "event")[case % 3]
        B, T_r, T_e = int(rng.integers(1, 71)), int(rng.integers(1, 301)), int(rng.integers(1, 46))
        W, L = int(rng.integers(1, 9)), int(rng.integers(2, 31))
        if mode not in handles:
            bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, max_batch=70)
            handles[mode] = (bc, bc.init_random_weights(seed=31 + case))
        bc, flat = handles[mode]
        raw, ev, _ = rv.synthetic.make_slab(B, T_r, T_e, seed=case, max_raw_pad=min(15, T_r - 1), max_event_pad=min(10, T_e - 1))
        tok, sc = bc.beam_search_prediction(_inputs(rv, mode, raw, ev), W, L)
        ctok, csc = cpu_port.run(bc.cfg.oracle_cfg(), 2, 7, rv.weights.pack(bc.cfg, flat), raw, ev, W, L)
        assert tok.shape == ctok.shape, (case, mode, B, T_r, T_e, W, L)
        _explain_mismatches(rv, oracle, bc, flat, mode, raw, ev, W, L, tok.numpy(), ctok, f"case {case} {mode} {(B, T_r, T_e, W, L)}", sc.numpy(), csc)
        g, lg = bc.greedy_search_prediction(_inputs(rv, mode, raw, ev), L)
        cg, clg = cpu_port.run(bc.cfg.oracle_cfg(), 2, 7, rv.weights.pack(bc.cfg, flat), raw, ev, 1, L, greedy=True)
        assert g.shape == cg.shape and np.abs(lg.numpy() - clg)[(g.numpy() == cg).all(axis=1)].max() < TOL
    for bc, _ in handles.values():
        bc.close()


@pytest.mark.parametrize("weights", ["keras", "emitting"])
@pytest.mark.parametrize("W", [5, 8, 1])
def test_maximum_shapes_against_c_port(rv, oracle, W, weights):
    """The library's limits at once: T_raw + T_event = 352 (all 11 resident row groups of the persistent decode in use),
    max_output_len 64, beam 5 (persistent decode) / 8 (per-step kernels) / 1, a slab larger than the CU count."""
    from oracle import cpu_port
    B, T_r, T_e, L = 300, 307, 45, 64
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=B, max_raw_len=T_r, max_event_len=T_e,
                       max_output_len=L)
    if weights == "keras":
        flat = rv.weights.init_weights(bc.cfg, seed=41)
        flat["b_fc"][bc.cfg.end_token] = 0.4 if W != 8 else 0.0
    else:
        flat = _emitting_flat(rv, bc.cfg, seed=41)
    bc.set_weights_flat(flat)
    raw, ev, _ = rv.synthetic.make_slab(B, T_r, T_e, seed=W)
    tok, sc = bc.beam_search_prediction((raw, ev), W, L)
    ctok, csc = cpu_port.run(bc.cfg.oracle_cfg(), 2, 7, rv.weights.pack(bc.cfg, flat), raw, ev, W, L)
    assert tok.shape == ctok.shape
    if weights == "emitting":
        _assert_calls_are_strings(rv, bc, tok, f"max shapes W={W}")
    _explain_mismatches(rv, oracle, bc, flat, "joint", raw, ev, W, L, tok.numpy(), ctok, f"max shapes W={W}/{weights}", sc.numpy(), csc)
    with pytest.raises(rv._capi.RavventHipError):
        bc.beam_search_prediction((raw, ev), W, L + 1)
    bc.close()


@pytest.mark.parametrize("W,Tr,Te", [(5, 300, 30), (3, 200, 30), (1, 40, 9), (5, 60, 12)])
def test_two_decoder_cells_on_the_matrix_pipe(rv, oracle, W, Tr, Te):
    """The reference's enc3/dec2 family (StackedRNNCells of two LSTMCells, basecaller.py:85-91) on the persistent decode in its two forms:
    the default since round 4 -- every product of both cells on the matrix pipe (cell 0 over [ctx' | h_1 | h_0] with the attention
    layer's h part folded in, cell 1's input product right after cell 0's gates, its recurrent product at the end of the step; split-f16
    operands) -- and packed fp32 FMAs (option matrix_cell = 0), against each other, the per-step kernels and the fp64 oracle: tokens,
    beam ids and parents identical, per-step logits within 1e-4 of fp64 and within 2e-5 of each other, at the three memory-length
    variants of the kernel, with a chunk that is mostly padding; greedy search too."""
    B, L = 7, 14
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=3, decoder_depth=2, max_batch=B,
                       max_raw_len=Tr, max_event_len=Te)
    flat = rv.weights.init_weights(bc.cfg, seed=60 + W, gain=1.5)
    flat["b_fc"][bc.cfg.end_token] = 0.3
    flat["dec_cells.1.W"][:, 9] *= 8.0; flat["dec_cells.1.U"][5, :] *= 1e-3; flat["dec_cells.0.U"][:, 200] *= 6.0     # outliers in the three split images
    bc.set_weights_flat(flat)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(B, Tr, Te, seed=W, max_raw_pad=min(15, Tr - 1), max_event_pad=min(10, Te - 1))
    raw[2, Tr // 3:] = 0.0
    bc.set_option("persist_taps", 1)
    bc.set_option("profile", 1)
    got = {}
    for form, (persist, mcell) in {"mx": (1, 1), "fma": (1, 0), "steps": (0, 1)}.items():
        bc.set_option("persistent_decode", persist); bc.set_option("matrix_cell", mcell)
        bc.reset_profile()
        tok, sc = bc.beam_search_prediction((raw, ev), W, L)
        assert ("dec_persist" in bc.profile()) == bool(persist)
        S = tok.shape[1]
        got[form] = [tok.numpy().copy(), sc.numpy().copy()]
        if persist:
            got[form] += [bc.get_tensor("chunk_steps").astype(int), bc.get_tensor("step_logits").reshape(S, B, W, 7).copy(),
                          bc.get_tensor("step_ids").reshape(S, B, W).copy(), bc.get_tensor("parent_ids").reshape(S, B, W).copy()]
    taps = {}
    otok, osc = oracle.beam_search(w, bc.cfg.oracle_cfg(), raw, ev, W, L, dtype=np.float64, taps=taps)
    tag = f"two cells W={W} T_m={Tr + Te}"
    twin = _twin_beam(oracle, w, bc.cfg.oracle_cfg(), raw, ev, W, L, taps, osc, tag)
    for form in ("mx", "fma", "steps"):
        assert got[form][0].shape == otok.shape and (got[form][0] == otok).all() and np.abs(got[form][1] - osc).max() < TOL, form
    _assert_twin(dict(scores=float(np.abs(got["steps"][1] - osc).max())), twin, f"{tag} steps")    # (tokens equal: no chunk left)
    assert (got["mx"][2] == got["fma"][2]).all()
    for form in ("mx", "fma"):
        tok, sc, cs, lg, ids, par = got[form]
        for b in range(B):
            n = cs[b]
            assert np.abs(lg[:n, b] - taps["step_logits"][:n, b]).max() < TOL, (form, b)
            assert (ids[:n, b] == taps["step_ids"][:n, b]).all() and (par[:n, b] == taps["parent_ids"][:n, b]).all(), (form, b)
        _assert_twin(_beam_errors(lg, None, ids, par, cs, sc, taps, osc)[0], twin, f"{tag} {form}")
    for b in range(B):
        n = got["mx"][2][b]
        assert np.abs(got["mx"][3][:n, b] - got["fma"][3][:n, b]).max() < 2e-5, b
    gtaps = {}
    og, olg = oracle.greedy_search(w, bc.cfg.oracle_cfg(), raw, ev, L, taps=gtaps)
    gtwin = _twin_greedy(oracle, w, bc.cfg.oracle_cfg(), raw, ev, L, og, olg, gtaps, f"{tag} greedy")
    for mcell in (1, 0):
        bc.set_option("persistent_decode", 1); bc.set_option("matrix_cell", mcell)
        g, glg = bc.greedy_search_prediction((raw, ev), L)
        assert g.shape == og.shape and (g.numpy() == og).all() and np.abs(glg.numpy() - olg).max() < TOL, mcell
        _assert_twin(_greedy_errors(g.numpy(), glg.numpy(), None, og, olg, gtaps)[0], gtwin, f"{tag} greedy matrix_cell={mcell}")
    bc.close()


@pytest.mark.parametrize("dec_depth,enc_depth", [(2, 3), (3, 2)])
def test_stacked_decoder_cells(rv, oracle, dec_depth, enc_depth):
    """decoder_depth > 1 (StackedRNNCells, basecaller.py:85-91): the reference's enc3/dec2 model family."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=enc_depth,
                       decoder_depth=dec_depth, max_batch=16)
    flat = bc.init_random_weights(seed=5)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(7, 44, 9, seed=dec_depth)
    bc.set_option("debug_taps", 1)
    g, lg = bc.greedy_search_prediction((raw, ev), 12)
    gtaps = {}
    og, olg = oracle.greedy_search(w, bc.cfg.oracle_cfg(), raw, ev, 12, taps=gtaps)
    assert g.shape == og.shape and (g.numpy() == og).all() and np.abs(lg.numpy() - olg).max() < TOL
    tag = f"stacked cells D={dec_depth} enc_depth {enc_depth}"
    _assert_twin(_greedy_errors(g.numpy(), lg.numpy(), None, og, olg, gtaps)[0],
                 _twin_greedy(oracle, w, bc.cfg.oracle_cfg(), raw, ev, 12, og, olg, gtaps, f"{tag} greedy"), f"{tag} greedy")
    for W, flash, nt in ((5, 1, 512), (3, 0, 0), (8, 1, 0), (4, 1, 256)):
        bc.set_option("flash_attend", flash)
        bc.set_option("attend_threads", nt)
        tok, sc = bc.beam_search_prediction((raw, ev), W, 12)
        taps = {}
        ot, osc = oracle.beam_search(w, bc.cfg.oracle_cfg(), raw, ev, W, 12, taps=taps)
        assert tok.shape == ot.shape and (tok.numpy() == ot).all() and np.abs(sc.numpy() - osc).max() < TOL
        S = ot.shape[1]
        # beam order inside a step: equal to the fp64 oracle's except on a chunk whose fp64 decode passes through a near-tie
        # (two of the W + 1 best candidates of a step closer than 1e-6, below what fp32 scores resolve)
        pid, lgt = bc.get_tensor("parent_ids").reshape(S, 7, W), bc.get_tensor("step_logits").reshape(S, 7, W, 7)
        for b in range(7):
            if (pid[:, b] == taps["parent_ids"][:, b]).all():
                assert np.abs(lgt[:, b] - taps["step_logits"][:, b]).max() < TOL
            else:
                gap = _near_tie_gap(oracle, taps["step_logits"][:, b], W, bc.cfg.oracle_cfg()["end_token"])
                assert gap < 1e-6, f"chunk {b}, beam {W}: beam order differs from fp64 with no near-tie (smallest gap {gap:.3e})"
        # (a chunk whose parents differ is compared up to that step; the scores of every chunk, as above: the tokens are equal)
        err, _ = _beam_errors(lgt, None, bc.get_tensor("step_ids").reshape(S, 7, W), pid, np.full(7, S), None, taps, osc)
        err["scores"] = float(np.abs(sc.numpy() - osc).max())
        _assert_twin(err, _twin_beam(oracle, w, bc.cfg.oracle_cfg(), raw, ev, W, 12, taps, osc, f"{tag} W={W}"), f"{tag} W={W} flash {flash}/{nt}")
    bc.close()


def test_fused_postprocessing_matches_host_form(rv):
    """rv_beam_search_calls == tokens_to_nuc_sequences + calc_prob_logits_beam_search_scores[:len(seq)]."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=64)
    flat = rv.weights.init_weights(bc.cfg, seed=3)
    flat["b_fc"][1] = 1.0                      # some early '^' so strings have different lengths
    bc.set_weights_flat(flat)
    raw, ev, _ = rv.synthetic.make_slab(40, 70, 12, seed=9)
    tok, sc = bc.beam_search_prediction((raw, ev), 5, 24)
    seqs_ref = bc.tokens_to_nuc_sequences(tok)
    probs_ref = rv.utils.calc_prob_logits_beam_search_scores(sc).numpy()
    seqs, probs = bc.beam_search_calls((raw, ev), 5, 24)
    assert seqs == seqs_ref
    for s, p, pr in zip(seqs, probs, probs_ref):
        assert len(p) == len(s) and np.abs(p - pr[:len(s)]).max(initial=0.0) < 1e-6
    ev1 = rv.evaluator.PerformanceEvaluator(bc, fused_postprocessing=True).run_slabs(raw, ev, np.zeros((40, 24), np.int64), chunk_size=64)
    ev0 = rv.evaluator.PerformanceEvaluator(bc, fused_postprocessing=False).run_slabs(raw, ev, np.zeros((40, 24), np.int64), chunk_size=64)
    assert [a for a, _ in ev1["nuc_preds"]] == [a for a, _ in ev0["nuc_preds"]]
    bc.close()


@pytest.mark.parametrize("depth,wide", [(2, -1), (4, -1), (3, 1), (4, 2), (8, 0)])
def test_asynchronous_calls_match_synchronous(rv, depth, wide):
    """rv_beam_search_submit* / collect*: several slabs in flight on the handle's contexts (own streams and buffers, shared
    weights) give byte-identical results to the synchronous calls -- host inputs, device inputs, the fused post-processing, tickets
    collected out of order; one slab too many is refused; weights cannot be replaced under calls in flight."""
    import torch
    bc, _ = _mk(rv, max_batch=40, max_raw_len=120, max_event_len=20, max_output_len=24)
    flat = _emitting_flat(rv, bc.cfg, seed=3)
    bc.set_weights_flat(flat)
    bc.set_option("wide_recurrence", wide)
    slabs = [rv.synthetic.make_slab(n, 120, 20, seed=n)[:2] for n in (40, 7, 33, 40, 1, 17, 40, 25, 40, 12)]
    ref = [bc.beam_search_prediction(x, 5, 24) for x in slabs]
    ref = [(t.numpy().copy(), s.numpy().copy()) for t, s in ref]
    ref_calls = [bc.beam_search_call_arrays(x, 5, 24) for x in slabs]
    bc.set_async_depth(depth)
    if wide >= 0:
        same = lambda got, want: got[0].shape == want[0].shape and (np.asarray(got[0].cpu()) == want[0]).all() and np.array_equal(np.asarray(got[1].cpu()), want[1])
    else:     # per-call choice of the recurrence form from the chunks in flight (40 alone: packed FMA; 4 x 40: matrix pipe): f32 rounding apart
        same = lambda got, want: got[0].shape == want[0].shape and (np.asarray(got[0].cpu()) == want[0]).all() and np.abs(np.asarray(got[1].cpu()) - want[1]).max() < 1e-5
    # host inputs, in order
    outs = list(bc.beam_search_stream(slabs, 5, 24))
    assert len(outs) == len(slabs) and all(same(o, r) for o, r in zip(outs, ref))
    # device inputs, collected out of order
    dev = [(torch.from_numpy(r).cuda(), torch.from_numpy(e).cuda()) for r, e in slabs]
    tickets = [bc.submit_beam_search(dev[i], 5, 24) for i in range(depth)]
    with pytest.raises(rv._capi.RavventHipError, match="uncollected"):
        bc.submit_beam_search(dev[0], 5, 24)                   # every context is busy
    with pytest.raises(rv._capi.RavventHipError, match="in flight"):
        bc.set_weights_flat(flat)
    for i in reversed(range(depth)):
        assert same(bc.collect(tickets[i]), ref[i]), i
    with pytest.raises(rv._capi.RavventHipError):
        bc.collect(tickets[0])                                  # collected already
    outs = list(bc.beam_search_stream(dev, 5, 24))
    assert all(same(o, r) for o, r in zip(outs, ref))
    # fused post-processing
    for got, want in zip(bc.beam_search_stream(slabs, 5, 24, calls=True), ref_calls):
        assert all(np.array_equal(g, w) if wide >= 0 or g.dtype.kind != "f" else np.abs(g - w).max() < 1e-5 for g, w in zip(got, want))
    # the synchronous call still works between asynchronous ones, and an empty slab passes through
    t = bc.submit_beam_search(slabs[0], 5, 24)
    t_empty = bc.submit_beam_search((slabs[0][0][:0], slabs[0][1][:0]), 5, 24) if depth > 2 else None
    mid = bc.beam_search_prediction(slabs[1], 5, 24) if depth > 3 else None
    assert same(bc.collect(t), ref[0])
    if t_empty is not None:
        assert bc.collect(t_empty)[0].shape[0] == 0
    if mid is not None:
        assert same(mid, ref[1])
    # a refused submit (slab larger than the handle's max_batch) leaves no context busy; closing a handle with calls in flight waits for them
    big = rv.synthetic.make_slab(41, 120, 20, seed=1)[:2]
    for _ in range(depth + 1):
        with pytest.raises(rv._capi.RavventHipError, match="outside"):
            bc.submit_beam_search(big, 5, 24)
    tickets = [bc.submit_beam_search(slabs[i], 5, 24) for i in range(depth)]
    assert same(bc.collect(tickets[0]), ref[0])
    bc.close()                                                  # depth - 1 slabs still in flight


def test_device_outputs_are_fresh_per_call(rv):
    """Device-input calls return fresh tensors like the reference (an evaluator may keep one result per slab in a list);
    buffer reuse is an explicit opt-in."""
    import torch
    bc, _ = _mk(rv)
    raw, ev, _ = rv.synthetic.make_slab(8, 64, 12, seed=2)
    raw2, ev2, _ = rv.synthetic.make_slab(8, 64, 12, seed=3)
    d = lambda a: torch.from_numpy(a).cuda()
    t1, s1 = bc.beam_search_prediction((d(raw), d(ev)), 5, 12)
    keep_t, keep_s = t1.cpu().numpy().copy(), s1.cpu().numpy().copy()
    t2, s2 = bc.beam_search_prediction((d(raw2), d(ev2)), 5, 12)
    assert (t1.cpu().numpy() == keep_t).all() and np.array_equal(s1.cpu().numpy(), keep_s)
    assert not np.array_equal(s2.cpu().numpy(), keep_s)
    g1, l1 = bc.greedy_search_prediction((d(raw), d(ev)), 12)
    keep_l = l1.cpu().numpy().copy()
    bc.greedy_search_prediction((d(raw2), d(ev2)), 12)
    assert np.array_equal(l1.cpu().numpy(), keep_l)
    bc.reuse_output_buffers = True                      # opt-in: views into one buffer per shape
    t3, _ = bc.beam_search_prediction((d(raw), d(ev)), 5, 12)
    t4, _ = bc.beam_search_prediction((d(raw2), d(ev2)), 5, 12)
    assert t3.data_ptr() == t4.data_ptr()
    bc.close()


def _emitting(rv, bc, seed=22):
    """Random weights biased to call bases (gain 3: the calls vary along a read instead of one homopolymer).  Untrained
    weights cannot call a read correctly; these tests check that the sharded and the single-GPU paths agree byte for byte."""
    flat = rv.weights.init_weights(bc.cfg, seed=seed, gain=3.0)
    flat["b_fc"][3:7] += 1.5
    flat["b_fc"][bc.cfg.end_token] -= 1.0
    bc.set_weights_flat(flat)
    return flat


def test_sharded_read_two_shards_in_one_process(rv):
    """BASELINE configs 4/5 on the one GPU of this box: a synthetic 8k-base read, its chunk range cut in two
    (`dist.shard_range`), the shards decoded one after the other, packed into the all-gather wire format, laid out
    rank-major as `all_gather_into_tensor` would, unpacked through the same read-order index and stitched by the C++
    merger == the single-GPU evaluator on the whole read."""
    bc, _ = _mk(rv, max_batch=256, max_raw_len=200, max_event_len=30, max_output_len=40)
    _emitting(rv, bc)
    sig, lab = rv.synthetic.make_read(8000, seed=11)
    ev = rv.evaluator.PerformanceEvaluator(bc, fused_postprocessing=True)
    whole = ev.run_read(sig, lab, chunk_size=256)
    assert whole["chunks_num"] > 1000 and len(whole["merged_seq"]) > 50
    dl = rv.data_loader
    lab_a = np.asarray(lab)
    raw_s, ev_s, nuc_s = dl.snippets_to_slab(*dl.prepare_snippets(sig, lab_a[:, :2].astype(int), lab_a[:, 2], 6))
    n, L = raw_s.shape[0], nuc_s.shape[1]
    for world in (2, 3):
        rows = []
        for rank in range(world):
            lo, hi = rv.dist.shard_range(n, rank, world)
            b, p, l = ev.decode_range(raw_s, ev_s, lo, hi, L, chunk_size=256)
            rows.append(rv.dist.pack_call_arrays(b, p, l, n, L - 1, world))
        gb, gp, gl = rv.dist.unpack_call_arrays(np.concatenate(rows, axis=0), n, L - 1, world)
        assert gb.shape == (n, L - 1) and (gl == [len(s) for s, _ in whole["nuc_preds"]]).all()
        assert ev.merger.merge_arrays(gb, gp, gl)[0] == whole["merged_seq"]
    bc.close()


def _gpu_rank(rank, world, port, q):
    import os, sys
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import ravvent_basecaller_amd as rv
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=64, max_raw_len=200, max_event_len=30,
                       max_output_len=40, device=0)
    flat = rv.weights.init_weights(bc.cfg, seed=22, gain=3.0)
    flat["b_fc"][3:7] += 1.5
    flat["b_fc"][bc.cfg.end_token] -= 1.0
    bc.set_weights_flat(flat)
    raw, ev, _ = rv.synthetic.make_slab(37, 64, 12, seed=5)
    out = {}
    t, s = rv.dist.sharded_beam_search(bc, raw, ev, 5, 14)                                   # host inputs
    out["host"] = (t.cpu().numpy(), s.cpu().numpy())
    t, s = rv.dist.sharded_beam_search(bc, torch.from_numpy(raw).cuda(), torch.from_numpy(ev).cuda(), 5, 14, slab=8)   # device inputs
    out["dev"] = (t.cpu().numpy(), s.cpu().numpy())
    t, s = rv.dist.sharded_beam_search(bc, raw[:1], ev[:1], 5, 14)                           # n < world: rank 1's shard is empty
    out["one"] = (t.cpu().numpy(), s.cpu().numpy())
    sig, lab = rv.synthetic.make_read(700, seed=4)
    res = rv.evaluator.PerformanceEvaluator(bc, fused_postprocessing=True).run_read_sharded(sig, lab, chunk_size=64)
    out["read"] = res["merged_seq"]
    if rank == 0:
        q.put(out)
    dist.barrier()
    bc.close()
    dist.destroy_process_group()


def test_sharded_two_ranks_on_one_gpu(rv):
    """The shipped multi-GPU path (dist.sharded_beam_search, evaluator.run_read_sharded) with the REAL Basecaller on two
    ranks that share this box's GPU (gloo moves the gather through host memory; RCCL refuses two ranks on one device):
    host inputs, device inputs with slab-split shards, a shard that is empty, and a read through shard -> gather -> merge."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 311) % 2000
    procs = [ctx.Process(target=_gpu_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    bc, _ = _mk(rv, max_batch=64, max_raw_len=200, max_event_len=30, max_output_len=40)
    _emitting(rv, bc)
    raw, ev, _ = rv.synthetic.make_slab(37, 64, 12, seed=5)
    t, s = bc.beam_search_prediction((raw, ev), 5, 14)
    for key in ("host", "dev"):
        assert out[key][0].shape == tuple(t.shape) and (out[key][0] == t.numpy()).all() and np.array_equal(out[key][1], s.numpy()), key
    t1, s1 = bc.beam_search_prediction((raw[:1], ev[:1]), 5, 14)
    assert (out["one"][0] == t1.numpy()).all() and np.array_equal(out["one"][1], s1.numpy())
    sig, lab = rv.synthetic.make_read(700, seed=4)
    single = rv.evaluator.PerformanceEvaluator(bc, fused_postprocessing=True).run_read(sig, lab, chunk_size=64)
    assert len(single["merged_seq"]) > 30 and out["read"] == single["merged_seq"]
    bc.close()


@pytest.mark.parametrize("B,Tr,Te,W,L", [(9, 120, 20, 5, 20), (6, 300, 30, 5, 24), (5, 40, 8, 1, 12), (4, 60, 0, 8, 14), (3, 307, 45, 3, 10), (7, 200, 30, 6, 16)])
def test_bahdanau_persistent_decode(rv, oracle, B, Tr, Te, W, L):
    """Bahdanau attention (Decoder(attention_type='bahdanau'), basecaller.py:131-132; north_star) on the one-launch persistent
    decode, in its two forms -- the default since round 4: tanh scores on the vector ALU, processed query h . W_q, context, cell product
    and output layer on the matrix pipe (split-f16 operands: option matrix_cell = 1); and everything on packed fp32 FMAs (matrix_cell =
    0) -- == the per-step kernels (exact reference dataflow: scores from keys, tanh, context from values) == the fp64 oracle; per-step
    logits of both persistent forms within 1e-4 of fp64 and within 2e-5 of each other, ids / parents identical; greedy logits within
    1e-4.  Weights scaled up (gain 1.5: larger keys and queries) and a chunk with most of its raw steps padded."""
    mode = "joint" if Te else "raw"
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, attention_type="bahdanau", honor_attention_type=True,
                       max_batch=16, max_raw_len=320)
    flat = rv.weights.init_weights(bc.cfg, seed=19, gain=1.5)
    flat["b_fc"][bc.cfg.end_token] = 0.5
    flat["W_q"][:, 7] *= 6.0; flat["W_q"][3, :] *= 1e-3          # an outlier column and a tiny row in the query layer's split image
    bc.set_weights_flat(flat)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(B, Tr, max(Te, 1), seed=B + W)
    raw[1, Tr // 2:] = 0.0
    x = (raw, ev) if mode == "joint" else raw
    out, lg, ids, par, cs, al = {}, {}, {}, {}, {}, {}
    bc.set_option("profile", 1)
    bc.set_option("persist_taps", 1)
    for form, (persist, mcell) in {"mx": (1, 1), "fma": (1, 0), "steps": (0, 1)}.items():
        bc.set_option("persistent_decode", persist)
        bc.set_option("matrix_cell", mcell)
        bc.reset_profile()
        tok, sc = bc.beam_search_prediction(x, W, L)
        assert ("dec_persist" in bc.profile()) == bool(persist)
        out[form] = (tok.numpy().copy(), sc.numpy().copy())
        if persist:
            S = tok.shape[1]
            lg[form] = bc.get_tensor("step_logits").reshape(S, B, W, 7).copy()
            ids[form] = bc.get_tensor("step_ids").reshape(S, B, W).copy()
            par[form] = bc.get_tensor("parent_ids").reshape(S, B, W).copy()
            cs[form] = bc.get_tensor("chunk_steps").astype(int)
            al[form] = bc.get_tensor("step_alignments").reshape(S, B, W, -1).copy()
    taps = {}
    ot, osc = oracle.beam_search(w, bc.cfg.oracle_cfg(), raw, ev if mode == "joint" else None, W, L, dtype=np.float64, taps=taps)
    r_, e_ = raw, ev if mode == "joint" else None
    tag = f"Bahdanau W={W} T_m={Tr + Te}"
    twin = _twin_beam(oracle, w, bc.cfg.oracle_cfg(), r_, e_, W, L, taps, osc, tag)
    for form in ("mx", "fma", "steps"):
        assert out[form][0].shape == ot.shape and (out[form][0] == ot).all() and np.abs(out[form][1] - osc).max() < TOL, form
    _assert_twin(dict(scores=float(np.abs(out["steps"][1] - osc).max())), twin, f"{tag} steps")    # (tokens equal: no chunk left)
    assert (cs["mx"] == cs["fma"]).all()
    for form in ("mx", "fma"):
        for b in range(B):
            n = cs[form][b]
            assert np.abs(lg[form][:n, b] - taps["step_logits"][:n, b]).max() < TOL, (form, b)
            assert (ids[form][:n, b] == taps["step_ids"][:n, b]).all() and (par[form][:n, b] == taps["parent_ids"][:n, b]).all(), (form, b)
    # alignments: the f16 image the context product consumes (mx: ATT 4), the fp32 rows (fma: ATT 1)
    worst = {form: _check_alignments(al[form], taps["step_alignments"], taps["mask"], cs[form], f"bahdanau {form}") for form in ("mx", "fma")}
    print(f"Bahdanau W={W} T_m={Tr + Te}: max |alpha - fp64|", worst)
    for form in ("mx", "fma"):
        _assert_twin(_beam_errors(lg[form], al[form], ids[form], par[form], cs[form], out[form][1], taps, osc)[0], twin, f"{tag} {form}")
    for b in range(B):
        n = cs["mx"][b]
        assert np.abs(lg["mx"][:n, b] - lg["fma"][:n, b]).max() < 2e-5, b
        assert np.abs(al["mx"][:n, b] - al["fma"][:n, b]).max() < 2e-5, b
    gtaps = {}
    og, olg = oracle.greedy_search(w, bc.cfg.oracle_cfg(), r_, e_, L, taps=gtaps)
    gtwin = _twin_greedy(oracle, w, bc.cfg.oracle_cfg(), r_, e_, L, og, olg, gtaps, f"{tag} greedy")
    for mcell in (1, 0):
        bc.set_option("persistent_decode", 1); bc.set_option("matrix_cell", mcell)
        g, glg = bc.greedy_search_prediction(x, L)
        assert g.shape == og.shape and (g.numpy() == og).all() and np.abs(glg.numpy() - olg).max() < TOL, mcell
        _assert_twin(_greedy_errors(g.numpy(), glg.numpy(), None, og, olg, gtaps)[0], gtwin, f"{tag} greedy matrix_cell={mcell}")
    bc.close()


@pytest.mark.parametrize("case", ["large_keys", "large_queries"])
def test_bahdanau_matrix_form_outside_the_fast_range(rv, oracle, case):
    """The Bahdanau decode's matrix-pipe form keeps E_k = 2^(2 log2(e) k) resident and takes a score element as 1 / (1 + E_k E_q): exact
    while |2 log2(e) k| <= 64 and |2 log2(e) q| <= 60.  Outside that range it must not clamp: a chunk with a larger key keeps the keys
    themselves and pays two transcendentals per element, a step with a larger processed query goes through log2(E_k).  Both regimes
    here (W_mem x 250: keys of several tens; W_q x 200: processed queries of several tens), against the packed-FMA form of the same
    library, which always computes tanh from k + q: chunk step counts equal, per-step logits within 1e-4 on every chunk whose
    beam order agrees (tanh is saturated almost everywhere, so near-ties are common), tokens equal on most rows; and the fp64 oracle
    agrees with the matrix form on every chunk it can be compared on."""
    B, Tr, Te, W, L = 10, 120, 20, 4, 10
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, attention_type="bahdanau", honor_attention_type=True,
                       max_batch=16, max_raw_len=Tr, max_event_len=Te)
    flat = rv.weights.init_weights(bc.cfg, seed=23)
    if case == "large_keys":
        flat["W_mem"] *= 250.0
    else:
        flat["W_q"] *= 200.0
    flat["b_fc"][bc.cfg.end_token] = -1.0
    bc.set_weights_flat(flat)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    raw, ev, _ = rv.synthetic.make_slab(B, Tr, Te, seed=6)
    taps, pq_max, orig_step = {}, [0.0], oracle.attention_step
    def spy(weights, *a, **k):                               # the largest |h . W_q| the fp64 decode sees
        out = orig_step(weights, *a, **k)
        pq_max[0] = max(pq_max[0], float(np.abs(out[3][-1][0] @ np.asarray(weights["W_q"], np.float64)).max()))
        return out
    oracle.attention_step = spy
    try:
        ot, osc = oracle.beam_search(w, bc.cfg.oracle_cfg(), raw, ev, W, L, dtype=np.float64, taps=taps)
    finally:
        oracle.attention_step = orig_step
    if case == "large_keys":
        assert np.abs(taps["keys"]).max(axis=(1, 2)).min() > 22.2      # |2 log2(e) k| > 64 somewhere in EVERY chunk's memory
    else:
        assert pq_max[0] > 25.0 and np.abs(taps["keys"]).max() < 22.0  # |2 log2(e) q| > 60 at some step, keys in range
    bc.set_option("persist_taps", 1)
    got = {}
    for mcell in (1, 0):
        bc.set_option("matrix_cell", mcell)
        tok, sc = bc.beam_search_prediction((raw, ev), W, L)
        S = tok.shape[1]
        got[mcell] = (tok.numpy().copy(), sc.numpy().copy(), bc.get_tensor("step_logits").reshape(S, B, W, 7).copy(),
                      bc.get_tensor("parent_ids").reshape(S, B, W).copy(), bc.get_tensor("chunk_steps").astype(int))
    assert np.isfinite(got[1][2][:1]).all() and got[1][0].shape == got[0][0].shape
    same_order = 0
    for b in range(B):
        n = min(got[1][4][b], got[0][4][b])
        if (got[1][3][:n, b] == got[0][3][:n, b]).all() and (got[1][0][b] == got[0][0][b]).all():
            same_order += 1
            assert np.abs(got[1][2][:n, b] - got[0][2][:n, b]).max() < TOL, (case, b)
    assert same_order >= B - 2, (case, same_order)
    n_cmp = 0
    for b in range(B):
        n = min(got[1][4][b], ot.shape[1])
        if (got[1][3][:n, b] == taps["parent_ids"][:n, b]).all():
            n_cmp += 1
            assert np.abs(got[1][2][:n, b] - taps["step_logits"][:n, b]).max() < TOL, (case, b)
    assert n_cmp >= B - 3, (case, n_cmp)
    bc.close()


@pytest.mark.parametrize("wide", [1, 0])
def test_chunks_never_interact_at_full_size(rv, wide):
    """Size-independent property at BASELINE's C3 size: a chunk decoded inside a 256-chunk slab (two rows per recurrence workgroup,
    one of 256 decode workgroups) and the same chunk decoded ALONE (one row per workgroup) give the same tokens and the same
    scores -- the per-row arithmetic does not depend on the slab around it; only the slab-wide step count S differs, and beyond
    a chunk's own last step the slab row holds the end token at an unchanged score."""
    B, T_r, T_e, W, L = 256, 300, 30, 5, 48
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=B, max_raw_len=T_r, max_event_len=T_e, max_output_len=L)
    flat = rv.weights.init_weights(bc.cfg, seed=22)
    flat["b_fc"][bc.cfg.end_token] = 0.3            # chunks stop at different steps
    bc.set_weights_flat(flat)
    bc.set_option("wide_recurrence", wide)          # matrix-pipe recurrence (16 chunks per workgroup) / packed-FMA kernels (2 rows per workgroup)
    raw, ev, _ = rv.synthetic.make_slab(B, T_r, T_e, seed=5)
    tok, sc = bc.beam_search_prediction((raw, ev), W, L)
    tok, sc = tok.numpy(), sc.numpy()
    end = bc.cfg.end_token
    for b in (0, 1, 2, 77, 128, 200, 254, 255):
        t1, s1 = bc.beam_search_prediction((raw[b:b + 1], ev[b:b + 1]), W, L)
        t1, s1 = t1.numpy()[0], s1.numpy()[0]
        n = t1.shape[0]
        assert n <= tok.shape[1] and (tok[b, :n] == t1).all() and np.array_equal(sc[b, :n], s1), b
        assert (tok[b, n:] == end).all() and (sc[b, n:] == s1[-1]).all(), b
    bc.close()
