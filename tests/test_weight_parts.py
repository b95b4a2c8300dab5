"""Option weight_parts 1 on the host: the rounding rule, that the GPU tests' inputs tell a rounded model from
the full one, and the bound the GPU test holds step 0 of the decode to.  No GPU: rv_round_weights needs no handle, the rest is the
fp64 oracle.

The rule, restated in numpy (round_columns): per column, s = the power of two that brings the column's largest |w| into
[2^13, 2^14) (2^14 for a zero column), w <- float16(w s) / s.  Blob-level tensors: U of every encoder layer and direction (128
rows), W of encoder layers >= 1 (256 rows), W_mem and rows u..3u-1 of W_att (256 rows).  The decoder's folded kernels are rounded
after their fold, by the loader; round_output_layer restates that for the output layer [W_fc ; A_h W_fc]."""
import numpy as np
import pytest

from test_split_image import _pack, special_weights


def round_columns(W):
    """[K][N] float32 -> each column rounded to the first f16 part of its split image."""
    W = np.asarray(W, np.float32)
    mx = np.abs(W).max(axis=0)
    _, ex = np.frexp(mx)
    ex = np.where((mx > 0) & np.isfinite(mx), ex, 0)
    s = np.ldexp(np.float32(1), 14 - ex).astype(np.float32)
    v = W * s                                                    # exact
    return (v.astype(np.float16).astype(np.float32) / s).astype(np.float32)


def is_rounded_name(name):
    """Whether the flat tensor `name` is a blob-level tensor the mode rounds as a whole (W_att is rounded in part: rows u..3u-1)."""
    if name == "W_mem":
        return True
    if not name.startswith("enc_"):
        return False
    _, layer, _, kind = name.split(".")                          # enc_<raw|event>.<layer>.<fwd|bwd>.<W|U|b>
    return kind == "U" or (kind == "W" and int(layer) >= 1)


def numpy_rounded_view(flat):
    out = {}
    for k, a in flat.items():
        a = np.asarray(a, np.float32)
        if is_rounded_name(k):
            out[k] = round_columns(a)
        elif k == "W_att":
            b = a.copy()
            b[128:384] = round_columns(a[128:384])
            out[k] = b
        else:
            out[k] = a.copy()
    return out


def pow2_scale(bound):
    """ravvent_hip.cpp, rv_load_weights: the power of two that brings `bound` (x 1.0001) into [2^13, 2^14)."""
    _, ex = np.frexp(float(bound) * 1.0001)
    return np.float32(np.ldexp(1.0, 14 - int(ex)))


def round_output_layer(flat):
    """The output layer as the mode's loader builds it from `flat` (whose A_c is rounded already): the fold [W_fc ; A_h W_fc] in
    fp64 -> float32, rows divided by the factor their input's f16 image carries (mx_uscale for the context rows, 2^14 for the h
    rows), one power-of-two scale Tl for the tensor, float16(w Tl) / Tl.  Returns (unrounded [256][V] float32, rounded [256][V])."""
    W_att, W_fc = np.asarray(flat["W_att"], np.float32), np.asarray(flat["W_fc"], np.float32)
    nh = (W_att[:128].astype(np.float64) @ W_fc.astype(np.float64)).astype(np.float32)
    w = np.concatenate([W_fc, nh], axis=0)
    uscale = pow2_scale(np.abs(W_att[128:384].astype(np.float64)).sum(axis=0).max())
    xs = np.concatenate([np.full(128, uscale, np.float32), np.full(128, 16384.0, np.float32)])[:, None]
    wl = w / xs                                                  # exact
    _, ex = np.frexp(np.abs(wl).max())
    Tl = np.float32(np.ldexp(1.0, 14 - int(ex)))
    r = ((wl * Tl).astype(np.float16).astype(np.float32) / Tl) * xs
    return w, r.astype(np.float32)


def _cfg(rv, mode="joint", enc_depth=2):
    return rv.config.RvConfig(enc_depth=enc_depth, mode=mode, max_batch=8, max_output_len=16)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("kind", ["ordinary", "special"])
@pytest.mark.parametrize("enc_depth", [1, 3])
def test_rounded_view_is_the_documented_rounding(rv, kind, enc_depth):
    cfg = _cfg(rv, enc_depth=enc_depth)
    flat = rv.weights.init_weights(cfg, seed=5 + enc_depth, gain=1.5)
    if kind == "special":
        rng = np.random.default_rng(9)
        for k in flat:
            if is_rounded_name(k):
                flat[k] = special_weights(rng, flat[k].shape[1])[:flat[k].shape[0]].copy()
        flat["W_att"][128:384] = special_weights(rng, 128)
    got = rv.weights.rounded_view(cfg, flat)
    want = numpy_rounded_view(flat)
    assert set(got) == set(flat)
    touched = 0
    for k in flat:
        assert got[k].shape == np.asarray(flat[k]).shape
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, "differs from the numpy restatement")
        if is_rounded_name(k) or k == "W_att":
            touched += 1
            assert not np.array_equal(_bits(got[k]), _bits(flat[k])), (k, "a tensor of the list came back unrounded")
        else:
            assert np.array_equal(_bits(got[k]), _bits(flat[k])), (k, "a tensor outside the list was touched")
    assert touched == 4 * enc_depth + 4 * (enc_depth - 1) + 2          # U: 2 encoders x 2 directions per layer; W from layer 1 on; W_mem, W_att
    assert np.array_equal(_bits(got["W_att"][:128]), _bits(flat["W_att"][:128]))      # A_h stays
    again = rv.weights.rounded_view(cfg, got)
    for k in flat:
        assert np.array_equal(_bits(again[k]), _bits(got[k])), (k, "not idempotent")


@pytest.mark.parametrize("kind", ["ordinary", "special"])
def test_rounding_is_the_first_part_of_the_packers_image(kind):
    """round_columns(W) == hi part x factor x 2^14 of rv_pack_split_image (through the probe library), and the image of the rounded
    kernel has that same first part and a zero second part."""
    rng = np.random.default_rng(3 + len(kind))
    W = (rng.standard_normal((256, 256)) * 0.08).astype(np.float32) if kind == "ordinary" else special_weights(rng, 256)
    img = _pack(W, 1)
    n = 2 * 256 * 256

    def parts(img):                                              # [ks][nt][part][lane = 16 kq + n][j] -> two [k][c] arrays
        a = img[:n].view(np.float16).reshape(8, 16, 2, 4, 16, 8).astype(np.float32)
        return [a[:, :, p].transpose(0, 2, 4, 1, 3).reshape(256, 256) for p in (0, 1)]    # (ks, kq, j | nt, n)
    f = img[n:].view(np.float32)
    hi, _ = parts(img)
    R = round_columns(W)
    assert np.array_equal(_bits(hi * (f * np.float32(2.0 ** 14))), _bits(R))
    img_r = _pack(R, 1)
    hi_r, lo_r = parts(img_r)
    fr = img_r[n:].view(np.float32)
    assert not lo_r.any(), "the second part of a rounded kernel's image is not zero"
    assert np.array_equal(_bits(hi_r * (fr * np.float32(2.0 ** 14))), _bits(R))


# ---- the oracle alone: what the GPU tests (tests/test_weight_parts_gpu.py) rest on

ENC_CASES = [("joint", 40, 12), ("joint", 200, 30)]


def enc_weights(rv, cfg):
    """Keras-default weights, seed 1 (the case the issue measured: 2.7e-5 / 3.3e-5 against a bound near 5e-6)."""
    return rv.weights.init_weights(cfg, seed=1)


def enc_slab(rv, Tr, Te, B=6):
    raw, ev, _ = rv.synthetic.make_slab(B, Tr, Te, seed=Tr, max_raw_pad=min(15, Tr - 1), max_event_pad=min(10, Te - 1))
    return raw, ev


@pytest.mark.parametrize("mode,Tr,Te", ENC_CASES)
def test_encoder_inputs_tell_the_rounded_model_from_the_full_one(rv, oracle, mode, Tr, Te):
    from test_parity_gpu import TWIN_C, TWIN_K
    cfg = _cfg(rv)
    flat = enc_weights(rv, cfg)
    raw, ev = enc_slab(rv, Tr, Te)
    w, wr = rv.weights.flat_to_nested(cfg, flat), rv.weights.flat_to_nested(cfg, rv.weights.rounded_view(cfg, flat))
    e64, _ = oracle.encode_input(w, raw, ev, mode, 0.0, np.float64)
    e32, _ = oracle.encode_input(w, raw, ev, mode, 0.0, np.float32)
    r64, _ = oracle.encode_input(wr, raw, ev, mode, 0.0, np.float64)
    bound = TWIN_K * float(np.abs(e32 - e64).max()) + TWIN_C
    moved = float(np.abs(r64 - e64).max())
    print(f"T_m={Tr + Te}: max |enc_output(rounded) - enc_output(full)| {moved:.2e}, twin bound {bound:.2e}, ratio {moved / bound:.1f}")
    assert moved >= 4 * bound, (moved, bound)


def step0(oracle, w, cfg, raw, ev, W=1):
    """Step 0 of the fp64 decode -> (logits [B,V], ctx' [B,128] = ctx . A_c, h [B,128])."""
    oc = cfg.oracle_cfg()
    enc, mask = oracle.encode_input(w, raw, ev, oc["mode"], 0.0, np.float64)
    keys, values = oracle.setup_memory(w, enc, mask, np.float64)
    B = enc.shape[0]
    z = np.zeros((B, 128))
    logits, _, alpha, st = oracle.attention_step(w, np.full(B, oc["start_token"], np.int32), z, [(z, z)], keys, values, mask, "luong", np.float64)
    h = st[-1][0]
    ctx = np.einsum("bt,bte->be", alpha, values)
    return logits, ctx @ np.asarray(w["W_att"], np.float64)[128:384], h


def step0_bound(flat_rounded, ctxp, h):
    """(logits of the rounded output layer on the oracle's own [ctx' | h], the bound 2^-11 sum_k |x_k| |w_k| per logit)."""
    w, r = round_output_layer(flat_rounded)
    x = np.concatenate([ctxp, h], axis=1)
    lg = x @ r.astype(np.float64) + np.asarray(flat_rounded["b_fc"], np.float64)
    return lg, 2.0 ** -11 * (np.abs(x) @ np.abs(w.astype(np.float64)))


def test_step0_bound_is_sound(rv, oracle):
    cfg = _cfg(rv)
    flat = rv.weights.init_weights(cfg, seed=70, gain=1.5)
    fr = rv.weights.rounded_view(cfg, flat)
    raw, ev = enc_slab(rv, 40, 12)
    logits, ctxp, h = step0(oracle, rv.weights.flat_to_nested(cfg, fr), cfg, raw, ev)
    lg_r, bound = step0_bound(fr, ctxp, h)
    diff = np.abs(lg_r - logits)
    print(f"step 0: max |logits(rounded output layer) - logits| {diff.max():.2e}, bound min {bound.min():.2e} max {bound.max():.2e}")
    assert (diff <= bound).all(), (diff.max(), bound.min())
    assert diff.max() > 1e-6, "the rounding of the output layer moves nothing: the bound would hold anything"
