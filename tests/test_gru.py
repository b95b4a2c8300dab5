"""rnn_type='bigru' without a GPU: the reference's formulas against torch.nn.GRU, the blob layout, the checkpoint import, the public
constructor, and the proof -- on the numpy reference alone -- that the inputs of tests/test_gru_gpu.py are fair probes."""
import numpy as np
import pytest

import gru_cases as C
import gru_reference as G


# ---------------------------------------------------------------------------------------------- the formulas
@pytest.mark.parametrize("F", [1, 5, 256])
def test_bigru_layer_is_torch_gru_in_fp64(F):
    """Keras GRUCell (reset_after=True, gates z, r, h) restated in gru_reference == torch.nn.GRU(bidirectional=True): gates permuted
    z, r, h -> r, z, n, weight = kernel.T, b_ih = b[0], b_hh = b[1]; both directions, both biases and both initial states non-zero."""
    import torch
    rng = np.random.default_rng(F)
    u, B, T = 128, 3, 7
    perm = np.r_[u:2 * u, 0:u, 2 * u:3 * u]
    cells = {d: (rng.standard_normal((F, 3 * u)) * 0.3, rng.standard_normal((u, 3 * u)) * 0.2, rng.standard_normal((2, 3 * u)) * 0.5)
             for d in ("fwd", "bwd")}
    x = rng.standard_normal((B, T, F))
    h0 = rng.uniform(-1, 1, (2, B, u))
    out, (hf, hb) = G.bigru_layer(x, cells["fwd"], cells["bwd"], (h0[0], h0[1]))
    gru = torch.nn.GRU(F, u, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for d, sfx in (("fwd", ""), ("bwd", "_reverse")):
            W, U, b = cells[d]
            getattr(gru, "weight_ih_l0" + sfx).copy_(torch.from_numpy(W[:, perm].T.copy()))
            getattr(gru, "weight_hh_l0" + sfx).copy_(torch.from_numpy(U[:, perm].T.copy()))
            getattr(gru, "bias_ih_l0" + sfx).copy_(torch.from_numpy(b[0, perm].copy()))
            getattr(gru, "bias_hh_l0" + sfx).copy_(torch.from_numpy(b[1, perm].copy()))
        tout, th = gru(torch.from_numpy(x), torch.from_numpy(h0))
    err = max(float(np.abs(out - tout.numpy()).max()), float(np.abs(hf - th[0].numpy()).max()), float(np.abs(hb - th[1].numpy()).max()))
    print(f"F={F}: max |reference - torch.nn.GRU| {err:.2e}")
    assert err < 1e-12


def test_stacked_layers_chain_their_final_states():
    """Layer l + 1 starts from layer l's two final states (Encoder.call): the encoder equals the layers called by hand."""
    rng = np.random.default_rng(0)
    u = 128
    cell = lambda F: (rng.standard_normal((F, 3 * u)) * 0.2, rng.standard_normal((u, 3 * u)) * 0.2, rng.standard_normal((2, 3 * u)) * 0.1)
    layers = [{"fwd": cell(5), "bwd": cell(5)}, {"fwd": cell(2 * u), "bwd": cell(2 * u)}]
    x = rng.standard_normal((2, 6, 5))
    o0, s0 = G.bigru_layer(x, layers[0]["fwd"], layers[0]["bwd"], None)
    o1, s1 = G.bigru_layer(o0, layers[1]["fwd"], layers[1]["bwd"], s0)
    out, st = G.encoder(x, layers)
    assert np.array_equal(out, o1) and all(np.array_equal(a, b) for a, b in zip(st, s1))
    assert not np.array_equal(o1, G.bigru_layer(o0, layers[1]["fwd"], layers[1]["bwd"], None)[0])


# ---------------------------------------------------------------------------------------------- the blob
@pytest.mark.parametrize("enc_depth", [1, 2, 3])
@pytest.mark.parametrize("dec_depth", [1, 2])
def test_bigru_blob_layout_and_round_trip(rv, enc_depth, dec_depth):
    W = rv.weights
    cfg = rv.config.RvConfig(enc_depth=enc_depth, dec_depth=dec_depth, rnn="bigru")
    u, d, V = 128, 128, 7
    layout = dict(W.blob_layout(cfg))
    for enc, F0 in (("raw", 1), ("event", 5)):
        for l in range(enc_depth):
            for dr in ("fwd", "bwd"):
                p = f"enc_{enc}.{l}.{dr}"
                assert (layout[p + ".W"], layout[p + ".U"], layout[p + ".b"]) == ((F0 if l == 0 else 2 * u, 3 * u), (u, 3 * u), (2, 3 * u))
    for k in range(dec_depth):
        p = f"dec_cells.{k}"
        assert (layout[p + ".W"], layout[p + ".U"], layout[p + ".b"]) == ((V + d if k == 0 else d, 3 * d), (d, 3 * d), (2, 3 * d))
    cells = sum(2 * ((F0 if l == 0 else 2 * u) * 3 * u + u * 3 * u + 2 * 3 * u) for F0 in (1, 5) for l in range(enc_depth))
    cells += sum((V + d if k == 0 else d) * 3 * d + d * 3 * d + 2 * 3 * d for k in range(dec_depth))
    rest = 2 * u * d + d * d + d + (d + 2 * u) * d + d * V + V
    assert W.blob_size(cfg) == cells + rest
    flat = W.init_weights(cfg, seed=3)
    for name, a in flat.items():
        if name.endswith(".b"):
            assert not a.any(), (name, "a GRU's biases start at zero: no forget gate")
        if name.endswith(".U"):
            assert np.abs(a @ a.T - np.eye(a.shape[0])).max() < 1e-5, (name, "orthogonal recurrent kernel")
    rng = np.random.default_rng(1)
    for name in flat:                                     # non-zero biases too: the round trip must keep both rows apart
        if name.endswith(".b"):
            flat[name] = rng.standard_normal(flat[name].shape).astype(np.float32)
    blob = W.pack(cfg, flat)
    assert blob.size == W.blob_size(cfg) and blob.dtype == np.float32
    back = W.unpack(cfg, blob)
    assert list(back) == [n for n, _ in W.blob_layout(cfg)] and all(np.array_equal(back[n], flat[n]) for n in flat)
    nested = W.flat_to_nested(cfg, back)
    assert len(nested["enc_raw"]) == enc_depth and len(nested["dec_cells"]) == dec_depth
    assert nested["enc_event"][0]["bwd"][2].shape == (2, 3 * u) and nested["dec_cells"][0][0].shape == (V + d, 3 * d)
    with pytest.raises(ValueError):
        W.pack(cfg, {**flat, "enc_raw.0.fwd.b": np.zeros(3 * u, np.float32)})


def test_bilstm_layout_is_unchanged(rv):
    W = rv.weights
    cfg = rv.config.RvConfig()
    assert cfg.rnn == "bilstm" and W.blob_layout(cfg) == W.blob_layout(rv.config.RvConfig(rnn="bilstm"))
    u, d, V = 128, 128, 7
    want = []
    for enc, F0 in (("raw", 1), ("event", 5)):
        for l in range(2):
            for dr in ("fwd", "bwd"):
                p = f"enc_{enc}.{l}.{dr}"
                want += [(p + ".W", (F0 if l == 0 else 2 * u, 4 * u)), (p + ".U", (u, 4 * u)), (p + ".b", (4 * u,))]
    want += [("dec_cells.0.W", (V + d, 4 * d)), ("dec_cells.0.U", (d, 4 * d)), ("dec_cells.0.b", (4 * d,))]
    want += [("W_mem", (2 * u, d)), ("W_q", (d, d)), ("v_att", (d,)), ("W_att", (d + 2 * u, d)), ("W_fc", (d, V)), ("b_fc", (V,))]
    assert W.blob_layout(cfg) == want
    b = W.init_weights(cfg, seed=22)["enc_raw.0.fwd.b"]
    assert b.shape == (4 * u,) and (b[u:2 * u] == 1).all() and not b[:u].any()      # the unit forget-gate bias stays
    assert not hasattr(cfg.to_c(), "rnn"), "the family is no part of the C record"
    with pytest.raises(ValueError):
        W.blob_layout(rv.config.RvConfig(rnn="gru"))


# ---------------------------------------------------------------------------------------------- checkpoint import
def test_gru_checkpoint_bundle_loads_into_the_flat_dict(rv, tmp_path):
    ck, W = rv.checkpoint, rv.weights
    cfg = rv.config.RvConfig(enc_depth=2, dec_depth=2, rnn="bigru", attention="bahdanau")
    flat = W.init_weights(cfg, seed=5)
    rng = np.random.default_rng(2)
    for name in flat:
        if name.endswith(".b"):
            flat[name] = rng.standard_normal(flat[name].shape).astype(np.float32)
    paths = ck.variable_paths(cfg)
    suffix = next(iter(ck.weights_manifest(cfg)))["checkpoint_key"][len(paths["enc_raw.0.fwd.W"]):]
    tensors = {paths[n] + suffix: a for n, a in flat.items()}
    ck.write_tensor_bundle(str(tmp_path / "gru"), tensors)
    got = ck.flat_from_checkpoint(str(tmp_path / "gru"), cfg)
    assert set(got) == set(flat) and all(np.array_equal(got[n], flat[n]) and got[n].shape == flat[n].shape for n in flat)
    assert np.array_equal(W.pack(cfg, got), W.pack(cfg, flat))
    # a reset_after=False model carries one bias row per cell: refused, by the variable's name
    key = paths["enc_event.1.bwd.b"] + suffix
    bad = {**tensors, key: np.zeros(3 * 128, np.float32)}
    with pytest.raises(ValueError) as e:
        ck.flat_from_tensors(bad, cfg)
    assert key in str(e.value) and "reset_after" in str(e.value) and "unsupported" in str(e.value)


# ---------------------------------------------------------------------------------------------- the public constructor
def test_bigru_constructor_reaches_the_library(rv):
    """rnn_type='bigru' is built: the constructor no longer raises NotImplementedError.  Without a GPU it gets as far as the library,
    which has no CPU path (RV_EHIP); with one it returns a handle of the GRU's weight count.  The unidirectional families still raise."""
    import torch
    try:
        bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, rnn_type="bigru", max_batch=4)
    except rv._capi.RavventHipError as e:
        assert not torch.cuda.is_available(), e
        assert "RV_EHIP" in str(e) and "rv_create_rnn" in str(e)
    else:
        assert bc.rnn_type == "bigru" and bc.cfg.rnn == "bigru"
        assert bc._lib.rv_weight_count(bc._h) == rv.weights.blob_size(bc.cfg)
        bc.close()
    for fam in ("gru", "lstm"):
        with pytest.raises(NotImplementedError):
            rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, rnn_type=fam)


# ---------------------------------------------------------------------------------------------- the GPU cases are fair probes
@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_gpu_case_inputs_meet_their_conditions(rv, name):
    """On the reference alone: the fp32 twin leaves the fp64 decode on at most B // 4 chunks (_stays, inside twin_errors), no chunk is
    padding from end to end unless the case says so, and the decode has steps to compare."""
    c, r = C.BY_NAME[name], C.fp64(rv, name)
    mask = r["taps"]["mask"]
    empty = [b for b in range(c.B) if not mask[b].any()]
    assert empty == ([] if c.all_pad is None else [c.all_pad]), (name, "chunks that are padding from end to end", empty)
    assert mask.shape == (c.B, {"raw": c.Tr, "event": c.Te, "joint": c.Tr + c.Te}[c.mode])
    S = r["out"][0].shape[1]
    assert S >= 2, (name, "the decode stops at once", S)
    twin = C.twin_errors(rv, name)
    print(f"{name}: S={S}, twin " + ", ".join(f"{k} {v:.1e}" for k, v in twin.items()))
    assert all(np.isfinite(v) for v in twin.values()), (name, twin)
    if c.all_pad is not None:
        assert S == c.L - 1, (name, "an all-padding chunk never finishes: the slab runs every step")
        lg = r["taps"]["step_logits"][:, c.all_pad] if c.W else r["out"][1][c.all_pad]
        assert np.isnan(lg).all() and np.isnan(r["taps"]["step_alignments"][:, c.all_pad]).all()


def test_case_biases_are_observable(rv):
    """The shared weights carry non-zero biases in both rows of every cell, and each way of getting them wrong moves the reference's
    tensors far beyond every tolerance of the GPU tests: biases dropped, rows 0 and 1 swapped, b[1]_h added outside the reset product."""
    c = C.WORLD
    flat, w = C.weights(rv, c.enc_depth, c.dec_depth, c.mode, c.attention)
    cells = [n for n in flat if n.endswith(".b")]
    assert len(cells) == 2 * 2 * c.enc_depth + c.dec_depth
    for n in cells:
        assert flat[n].shape[0] == 2 and (np.abs(flat[n]) > 0).all(axis=1).all() and np.abs(flat[n]).std() > 0.1, n
    r = C.fp64(rv, c.name)
    cfg = C.config(rv, c)
    for what, change in (("dropped", lambda b: np.zeros_like(b)), ("rows swapped", lambda b: b[::-1].copy())):
        wrong = rv.weights.flat_to_nested(cfg, {n: (change(a) if n.endswith(".b") else a) for n, a in flat.items()})
        enc, _ = G.encode_input(wrong, r["raw"], r["ev"], c.mode)
        lg, *_ = G.attention_step(wrong, np.full((c.B,), 2), np.zeros((c.B, 128)), [np.zeros((c.B, 128))] * c.dec_depth,
                                  r["taps"]["keys"], r["taps"]["enc_output"] * r["taps"]["mask"][..., None], r["taps"]["mask"], c.attention, np.float64)
        right, *_ = G.attention_step(w, np.full((c.B,), 2), np.zeros((c.B, 128)), [np.zeros((c.B, 128))] * c.dec_depth,
                                     r["taps"]["keys"], r["taps"]["enc_output"] * r["taps"]["mask"][..., None], r["taps"]["mask"], c.attention, np.float64)
        d_enc, d_lg = float(np.abs(enc - r["taps"]["enc_output"]).max()), float(np.abs(lg - right).max())
        print(f"biases {what}: enc_output moves by {d_enc:.2e}, first-step logits by {d_lg:.2e}")
        assert d_enc > 1e-2 and d_lg > 1e-3, (what, d_enc, d_lg)
    # b[1]_h outside the reset product, on layer 0 of the raw encoder: h' of one step from a non-zero state
    W, U, b = (np.asarray(a, np.float64) for a in w["enc_raw"][0]["fwd"])
    rng = np.random.default_rng(0)
    x, h, u = rng.standard_normal((4, 1)), rng.uniform(-1, 1, (4, 128)), 128
    xi, hr = x @ W + b[0], h @ U + b[1]
    rr = G._sigmoid(xi[:, u:2 * u] + hr[:, u:2 * u])
    z = G._sigmoid(xi[:, :u] + hr[:, :u])
    outside = np.tanh(xi[:, 2 * u:] + rr * (hr[:, 2 * u:] - b[1, 2 * u:]) + b[1, 2 * u:])
    d = float(np.abs((z * h + (1 - z) * outside) - G.gru_cell(x, h, W, U, b)).max())
    print(f"b[1]_h outside r * (.): h' moves by {d:.2e}")
    assert d > 1e-2


# ---------------------------------------------------------------------------------------------- the adversarial weights reach their regime
@pytest.mark.parametrize("saturate", [False, True], ids=["plain", "saturated"])
@pytest.mark.parametrize("col_gain", C.ADV_GAINS)
def test_adversarial_encoder_recipe_reaches_its_regime(rv, col_gain, saturate):
    """On the reference alone: with saturation more than 0.3 of |enc_output| lies within 2^-20 of 1 (the 2^14 image of h at its edge);
    without it the gained columns' recurrent pre-activations exceed 10 somewhere.  |h| <= 1 in fp64 and in the twin's own arithmetic,
    and the twin's error is finite: the probe is one an honest fp32 evaluation passes."""
    a = C.adversarial_encoder(rv, col_gain, saturate)
    print(f"adversarial encoder gain {col_gain:g} {'saturated' if saturate else 'plain'}: saturated share {a['saturated']:.3f}, "
          f"largest gained pre-activation {a['preact']:.1f}, twin enc_output {a['twin']['enc_output']:.1e} keys {a['twin']['keys']:.1e}")
    assert np.abs(a["enc_output"]).max() <= 1.0 and a["mask"].any(axis=1).all()
    if saturate:
        assert a["saturated"] > 0.3, a["saturated"]
    else:
        assert a["preact"] > 10.0, a["preact"]
    assert all(np.isfinite(v) for v in a["twin"].values())


@pytest.mark.parametrize("dec_depth", [1, 2])
def test_adversarial_decoder_recipe_is_a_fair_probe(rv, dec_depth):
    """On the reference alone: every chunk runs all L - 1 steps, and the fp32 twin leaves the fp64 beam on at most B // 4 chunks (_stays,
    inside adversarial_decoder) at the L of ADV_DEC; the gained h columns' recurrent pre-activations reach tens."""
    a = C.adversarial_decoder(rv, dec_depth)
    c = a["case"]
    assert a["taps"]["step_ids"].shape[0] == c.L - 1 and c.L <= 16
    print(f"adversarial decoder dec_depth {dec_depth}: twin " + ", ".join(f"{k} {v:.1e}" for k, v in a["twin"].items()))
    assert all(np.isfinite(v) for v in a["twin"].values())
