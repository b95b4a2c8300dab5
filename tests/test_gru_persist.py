"""The persistent GRU decode (option gru_persistent, k_dec_persist_gru) on the CPU.

  images    build_gru_persist_images of csrc/weight_images.cpp, dumped by tests/kernels/gru_persist_dump.cpp, against a numpy fp64 folding
            of the same blob (gru_persist_cases.fold_fp64).  The fragment images are unpacked by index maps that are first held to
            tests/test_split_image.py's restatement of the fragment order (numpy_image);
  tiling    the four-tile product [ctx' | h] . K + token row + bias and the kernel's gate formula equal tests/gru_reference.py's decoder
            step -- gru_cell on [one_hot | h_prev . A_h + ctx'] -- in fp64, both bias rows non-zero;
  bias      b[1]_h moved out of the reset product moves h' by more than 1e-2 (the argument of tests/test_gru.py);
  probes    every GPU case of tests/test_gru_persist_gpu.py that tests/gru_cases.py does not already hold is a fair probe on the
            reference alone: no all-padding chunk, at least two steps, and the fp32 twin on the fp64 decode on EVERY chunk."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gru_cases as C
import gru_persist_cases as P
import gru_reference as G
from test_split_image import numpy_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc")
V = 7


# ---------------------------------------------------------------------------------------------- fragment order
def unpack_split(img):
    """[8 k-steps][16 tiles][2 parts][64 lanes][8] -> (hi, lo) [256][256]: lane (n, kq) of tile nt, k-step ks holds W[32 ks + 8 kq + j][16 nt + n]."""
    a = np.asarray(img, np.uint16).reshape(8, 16, 2, 4, 16, 8).transpose(2, 0, 3, 5, 1, 4).reshape(2, 256, 256)
    return a[0].view(np.float16).astype(np.float64), a[1].view(np.float16).astype(np.float64)


def unpack_gate_pairs(img):
    """Wc16's order, [8 waves][32 pairs = 4 ks + gate][2 parts][64 lanes][8] -> (hi, lo) [256][512]: lane (n, kq) of wave wv, pair
    (ks, gate) holds K[32 ks + 8 kq + j][128 gate + 16 wv + n]."""
    a = np.asarray(img, np.uint16).reshape(8, 8, 4, 2, 4, 16, 8).transpose(3, 1, 4, 6, 2, 0, 5).reshape(2, 256, 512)
    return a[0].view(np.float16).astype(np.float64), a[1].view(np.float16).astype(np.float64)


def unpack_ksteps(img, waves):
    """[waves][k-steps][2 parts][64 lanes][8] -> (hi, lo) [32 k-steps'][16 waves]: Wl16 (one 16-column tile, 8 k-steps) and Wq16 (8 waves, 4)."""
    ks = img.size // (waves * 1024)
    a = np.asarray(img, np.uint16).reshape(waves, ks, 2, 4, 16, 8).transpose(2, 1, 3, 5, 0, 4).reshape(2, 32 * ks, 16 * waves)
    return a[0].view(np.float16).astype(np.float64), a[1].view(np.float16).astype(np.float64)


def test_the_unpackers_follow_the_restated_fragment_order():
    """unpack_split inverts test_split_image.numpy_image; the other two unpackers are the same lane map (row 8 kq + j of a k-step,
    column n of a 16-column tile) under their images' outer orders, shown one entry at a time on an image written by that map."""
    rng = np.random.default_rng(1)
    W = (rng.standard_normal((256, 256)) * 0.1).astype(np.float32)
    img = numpy_image(W, 1)
    f = img[2 * 256 * 256:].view(np.float32).astype(np.float64)
    hi, lo = unpack_split(img[:2 * 256 * 256])
    assert np.abs((hi + lo) * f * 2.0 ** 14 - W).max() <= np.abs(W).max() * 2.0 ** -21
    for k, c in ((0, 0), (7, 15), (8, 16), (37, 129), (255, 511), (130, 300)):
        ks, kq, j, g, wv, n = k // 32, (k % 32) // 8, k % 8, c // 128, (c % 128) // 16, c % 16
        img = np.zeros(8 * 32 * 1024, np.uint16)
        img[((wv * 32 + 4 * ks + g) * 2) * 512 + (16 * kq + n) * 8 + j] = np.float16(3.0).view(np.uint16)
        img[((wv * 32 + 4 * ks + g) * 2 + 1) * 512 + (16 * kq + n) * 8 + j] = np.float16(0.5).view(np.uint16)
        hi, lo = unpack_gate_pairs(img)
        assert hi[k, c] == 3.0 and lo[k, c] == 0.5 and np.count_nonzero(hi) == 1 and np.count_nonzero(lo) == 1, (k, c)


# ---------------------------------------------------------------------------------------------- images against numpy
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = tmp_path_factory.mktemp("gpd") / "gru_persist_dump"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "-Wall", "-x", "c++", "-I", CSRC, os.path.join(ROOT, "tests", "kernels", "gru_persist_dump.cpp"),
                    os.path.join(CSRC, "weight_images.cpp"), "-o", str(exe)], check=True, capture_output=True)
    return str(exe)


def _pow2_scale(mx):
    """split_image.h, rv_column_scale: the power of two that brings mx into [2^13, 2^14); 2^14 for zero."""
    _, ex = np.frexp(np.float32(mx))
    return float(np.ldexp(1.0, 14 - (int(ex) if mx > 0 else 0)))


@pytest.mark.parametrize("attention", ["luong", "bahdanau"])
def test_images_against_a_numpy_fp64_folding(rv, dump, tmp_path, attention):
    flat, _ = C.weights(rv, 2, 1, "joint", attention)
    cfg = rv.config.RvConfig(enc_depth=2, dec_depth=1, mode="joint", attention=attention, rnn="bigru", vocab=V)
    blob = str(tmp_path / "blob.bin")
    rv.weights.pack(cfg, flat).tofile(blob)
    r = subprocess.run([dump, blob, str(tmp_path), "2", str(rv.config.ATTENTIONS[attention]), str(V)], check=True, capture_output=True, text=True)
    sizes = {f[1]: (int(f[2]), int(f[3])) for f in (ln.split() for ln in r.stdout.splitlines()) if f[0] == "size"}
    sc = {f[1]: float.fromhex(f[2]) for f in (ln.split() for ln in r.stdout.splitlines()) if f[0] == "scale"}
    img = {k: np.fromfile(str(tmp_path / f"{k}.bin"), {2: np.uint16, 4: np.float32}[e]) for k, (e, n) in sizes.items()}
    assert set(img) == {"gWmp", "gWmp16", "gWkp16", "gWc16", "gWl16", "gWq16", "gWtok", "gbdec"} and all(img[k].size == sizes[k][1] for k in img)
    assert not any(k.startswith("W") for k in img), "new names: the X table of a bigru load holds no Wc16 and must not grow one"
    ref = P.fold_fp64(flat, V)
    # fp32 tensors: exact copies / one fp32 sum
    assert np.array_equal(img["gWmp"].reshape(256, 256), ref["mem"].astype(np.float32))
    tok = img["gWtok"].reshape(8, 512)
    assert np.array_equal(tok[:V], ref["tok"].astype(np.float32)) and not tok[V:].any() and not tok[:, 384:].any()
    b = np.asarray(flat["dec_cells.0.b"], np.float32)
    want_b = np.concatenate([b[0, :256] + b[1, :256], b[0, 256:], b[1, 256:]])
    assert np.array_equal(img["gbdec"], want_b) and np.abs(img["gbdec"][384:]).min() > 0
    # the memory kernel's split image: byte for byte what test_split_image restates, and Wkp16 a permutation of its W_mem half
    assert np.array_equal(img["gWmp16"], numpy_image(ref["mem"].astype(np.float32), 1))
    assert sorted(img["gWkp16"].reshape(-1, 8).tolist()) == sorted(img["gWmp16"][:2 * 256 * 256].reshape(8, 16, 2, 64, 8)[:, :8].reshape(-1, 8).tolist())
    # the folded kernel: rows divided by what their input's image carries (ctx': uscale, h: 2^14), one power-of-two scale T.  Two f16
    # parts hold a scaled value v to |v| 2^-22 (11 + 11 bits) or half the smallest f16 subnormal, 2^-25; the fp32 rounding of the fold
    # adds |v| 2^-24: bound |v| 2^-21 + 2^-24 in scaled units
    xs = np.where(np.arange(256) < 128, sc["uscale"], 16384.0)[:, None]
    Ks = ref["K"] / xs
    T = _pow2_scale(np.abs(Ks.astype(np.float32)).max())
    assert sc["cdescale"] == 1.0 / T
    hi, lo = unpack_gate_pairs(img["gWc16"])
    d = np.abs((hi + lo) - Ks * T)
    assert (d <= np.abs(Ks * T) * 2.0 ** -21 + 2.0 ** -24).all(), float(d.max())
    assert not hi[:128, 384:].any() and not lo[:128, 384:].any(), "ctx' rows of the fourth tile: the reset product sees h . U_h alone"
    assert np.abs(hi).max() >= 2.0 ** 13 and np.abs(hi).max() < 2.0 ** 14
    # the output layer on [ctx' | h], columns >= V zero
    Ls = ref["out"] / xs
    Tl = _pow2_scale(np.abs(Ls.astype(np.float32)).max())
    assert sc["ldescale"] == 1.0 / Tl
    hi, lo = unpack_ksteps(img["gWl16"], 1)
    d = np.abs((hi + lo)[:, :V] - Ls * Tl)
    assert (d <= np.abs(Ls * Tl) * 2.0 ** -21 + 2.0 ** -24).all() and not hi[:, V:].any() and not lo[:, V:].any()
    # Bahdanau's query layer
    Wq = np.asarray(flat["W_q"], np.float64)
    Tq = _pow2_scale(np.abs(Wq).max())
    assert sc["qdescale"] == 2.0 ** -14 / Tq
    hi, lo = unpack_ksteps(img["gWq16"], 8)
    assert (np.abs((hi + lo) - Wq * Tq) <= np.abs(Wq * Tq) * 2.0 ** -21 + 2.0 ** -24).all()
    # the memory scales: the bound-based powers of two of the LSTM forms
    for name, cols in (("kscale", slice(0, 128)), ("uscale", slice(128, 256))):
        bound = np.abs(ref["mem"].astype(np.float32).astype(np.float64)[:, cols]).sum(axis=0).max() * 1.0001
        assert 2.0 ** 13 <= bound * sc[name] < 2.0 ** 14, name


# ---------------------------------------------------------------------------------------------- tiling and bias placement
def _step_inputs(rv, attention):
    flat, w = C.weights(rv, 1, 1, "joint", attention)
    rng = np.random.default_rng(3)
    n = 9
    tok = rng.integers(0, V, n)
    h_prev, ctx_prev = rng.uniform(-1, 1, (n, 128)), rng.standard_normal((n, 128))
    return flat, w, tok, h_prev, ctx_prev


@pytest.mark.parametrize("attention", ["luong", "bahdanau"])
def test_the_four_tiles_and_the_gate_formula_equal_the_reference_cell(rv, attention):
    """The attention vector of the previous step is h_prev . A_h + ctx'_prev; the reference's cell takes [one_hot | attention] and the
    cell's own previous h, which with one cell is that same h_prev: h . U and h . A_h W_a share the kernel's h rows."""
    flat, w, tok, h_prev, ctx = _step_inputs(rv, attention)
    f = P.fold_fp64(flat, V)
    W, U, b = (np.asarray(a, np.float64) for a in w["dec_cells"][0])
    assert (np.abs(b) > 0).all(), "both bias rows non-zero"
    A = np.asarray(flat["W_att"], np.float64)
    att = h_prev @ A[:128] + ctx
    want = G.gru_cell(np.concatenate([np.eye(V)[tok], att], axis=-1), h_prev, W, U, b)
    z4 = np.concatenate([ctx, h_prev], axis=-1) @ f["K"] + f["tok"][tok] + f["bias"]
    got = P.gates(z4, h_prev)
    d = float(np.abs(got - want).max())
    print(f"{attention}: four tiles + gates against gru_cell: {d:.2e}")
    assert d < 1e-12
    # ... and the output layer on [ctx' | h] is the reference's attention layer followed by the output layer
    lg = np.concatenate([ctx, h_prev], axis=-1) @ f["out"] + np.asarray(flat["b_fc"], np.float64)
    assert np.abs(lg - (att @ np.asarray(flat["W_fc"], np.float64) + np.asarray(flat["b_fc"], np.float64))).max() < 1e-12


def test_b1h_outside_the_reset_product_is_observable(rv):
    flat, w, tok, h_prev, ctx = _step_inputs(rv, "luong")
    f = P.fold_fp64(flat, V)
    wrong = f["bias"].copy()
    wrong[256:384] += wrong[384:]                                     # b[1]_h beside b[0]_h, outside r * (.)
    wrong[384:] = 0.0
    x = np.concatenate([ctx, h_prev], axis=-1) @ f["K"] + f["tok"][tok]
    d = float(np.abs(P.gates(x + wrong, h_prev) - P.gates(x + f["bias"], h_prev)).max())
    print(f"b[1]_h outside r * (.): h' moves by {d:.2e}")
    assert d > 1e-2


# ---------------------------------------------------------------------------------------------- fair probes
@pytest.mark.parametrize("name", [c.name for c in P.NEW_CASES])
def test_new_gpu_cases_are_fair_probes(rv, name):
    c, r = P.BY_NAME[name], P.fp64(rv, name)
    mask = r["taps"]["mask"]
    assert [b for b in range(c.B) if not mask[b].any()] == [], (name, "chunks that are padding from end to end")
    S = r["out"][0].shape[1]
    assert S >= 2, (name, "the decode stops at once", S)
    left = P.twin_left(rv, name)
    assert left == [], (name, "the numpy fp32 twin leaves the fp64 decode on chunks: pick another slab seed", left)
    twin = P.twin_errors(rv, name)
    print(f"{name}: S={S}, twin " + ", ".join(f"{k} {v:.1e}" for k, v in twin.items()))
    assert all(np.isfinite(v) for v in twin.values()), (name, twin)


def test_every_form_of_the_list_has_a_case():
    forms = {P.form(c) for c in P.BY_NAME.values()}
    assert forms == {(11, W, nit, 1, att) for W in range(1, 9) for nit in (2, 8, 11) for att in (3, 4)}
