"""The weight images of csrc/weight_images.cpp, on the CPU: the stand-alone program tests/kernels/wimg_dump.cpp builds them from a blob
without a handle or a device.  Held here: every image's SHA-256 and the six weight-derived scalars against tests/golden/weight_images.json
(recorded from the packing loops as they stood inside rv_load_weights, carried over verbatim, before they were merged: run this file with
--record only to add a configuration); every image's size against the count rv_create_rnn allocates; the images that go through the shared
fragment writer of csrc/split_image.h byte for byte against numpy restatements of the layouts csrc/common.h documents; and the one
walk of the blob against weights.py and against test_weight_parts.numpy_rounded_view.

Blobs: weights.init_weights(scheme='hash') -- the generator behind Basecaller.init_random_weights without a handle, in the scheme that
regenerates bit for bit anywhere (the Keras scheme runs a LAPACK QR) -- with the special columns of test_split_image.special_weights
put into one U, one layer-1 W, W_mem and A_c."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "weight_images.json")

# name: (rnn, encoder depth, decoder depth, attention, vocab, weight_parts)
CONFIGS = {
    "bilstm-2-1-luong": ("bilstm", 2, 1, "luong", 7, 2),
    "bilstm-2-1-luong-parts1": ("bilstm", 2, 1, "luong", 7, 1),
    "bilstm-2-1-bahdanau": ("bilstm", 2, 1, "bahdanau", 7, 2),
    "bilstm-3-2-vocab5": ("bilstm", 3, 2, "luong", 5, 2),
    "bilstm-1-3": ("bilstm", 1, 3, "bahdanau", 7, 2),          # no layer >= 1 images, no fold
    "bigru-2-1-vocab6": ("bigru", 2, 1, "luong", 6, 2),
    "bigru-1-2": ("bigru", 1, 2, "bahdanau", 7, 2),            # no gWx16
}


def _cfg(name):
    import ravvent_basecaller_amd as rv
    rnn, enc, dec, att, vocab, _ = CONFIGS[name]
    return rv.config.RvConfig(enc_depth=enc, dec_depth=dec, attention=att, vocab=vocab, rnn=rnn)


def special_columns(seed, rows, N):
    """[rows][N] weights with, by column c % 16: 3 -> the column x 2^20, 5 -> x 2^-20, 7 -> a zero column, 11 -> the column's largest |w|
    exactly a power of two, 13 -> the float just below one (test_split_image.special_weights, for any row count and from splitmix64)."""
    from ravvent_basecaller_amd.weights import _splitmix_uniform
    W = (_splitmix_uniform(seed, rows * N).reshape(rows, N) * 0.14).astype(np.float32)
    c = np.arange(N)
    W[:, c % 16 == 3] *= np.float32(2.0 ** 20)
    W[:, c % 16 == 5] *= np.float32(2.0 ** -20)
    W[:, c % 16 == 7] = 0.0
    for j in c[(c % 16 == 11) | (c % 16 == 13)]:
        p = np.float32(2.0 ** ((j // 16) % 5 - 3))
        k = int(np.argmax(np.abs(W[:, j])))
        W[:, j] *= np.float32(0.4) * p / np.abs(W[k, j])         # everything else well below p
        W[k, j] = np.copysign(p if j % 16 == 11 else np.nextafter(p, np.float32(0)), W[k, j])
    return W


def make_flat(name):
    from ravvent_basecaller_amd import weights
    cfg = _cfg(name)
    flat = weights.init_weights(cfg, seed=100 + list(CONFIGS).index(name), scheme="hash")
    g = 3 if cfg.rnn == "bigru" else 4
    last = cfg.enc_depth - 1
    for i, k in enumerate(sorted(flat)):                         # biases that tell their rows and directions apart
        if k.startswith("enc_") and k.endswith(".b"):
            flat[k] = (weights._splitmix_uniform(50 + i, flat[k].size).reshape(flat[k].shape) * 0.5).astype(np.float32)
    flat[f"enc_event.{last}.bwd.U"] = special_columns(1, 128, 128 * g)
    if cfg.enc_depth > 1:
        flat["enc_raw.1.fwd.W"] = special_columns(2, 256, 128 * g)
    flat["W_mem"] = special_columns(3, 256, 128)
    flat["W_att"][128:] = special_columns(4, 256, 128)
    return cfg, flat


def _has_f16c():
    try:
        return "f16c" in open("/proc/cpuinfo").read().split()
    except OSError:
        return False


@pytest.fixture(scope="module", params=["soft-float", "f16c"])
def dump(request, tmp_path_factory):
    """The dump program, built both ways csrc/Makefile builds weight_images.o: half conversions as soft-float calls, and as F16C
    instructions where the host has them.  Both must give the same bytes."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    if request.param == "f16c" and not _has_f16c():
        pytest.skip("no F16C on this host: csrc/Makefile builds the soft-float form")
    exe = tmp_path_factory.mktemp("wimg") / "wimg_dump"
    subprocess.run(["hipcc", "-O3"] + (["-mf16c"] if request.param == "f16c" else []) +
                   ["-std=c++17", "-Wall", "-x", "c++", "-I", CSRC, os.path.join(ROOT, "tests", "kernels", "wimg_dump.cpp"),
                    os.path.join(CSRC, "weight_images.cpp"), "-o", str(exe)], check=True, capture_output=True)
    return str(exe)


def run_images(exe, name, out_dir):
    """wimg_dump images on configuration `name`: (blob floats, {image: (element bytes, elements)}, {scale: hex}, {image: bytes})."""
    from ravvent_basecaller_amd import config, weights
    cfg, flat = make_flat(name)
    os.makedirs(out_dir, exist_ok=True)
    blob = os.path.join(out_dir, "blob.bin")
    weights.pack(cfg, flat).tofile(blob)
    r = subprocess.run([exe, "images", blob, str(out_dir), str(config.RNNS[cfg.rnn]), str(cfg.enc_depth), str(cfg.dec_depth),
                        str(config.ATTENTIONS[cfg.attention]), str(cfg.vocab), str(CONFIGS[name][5])], check=True, capture_output=True, text=True)
    total, sizes, scales = None, {}, {}
    for ln in r.stdout.splitlines():
        f = ln.split()
        if f[0] == "total":
            total = int(f[1])
        elif f[0] == "size":
            sizes[f[1]] = (int(f[2]), int(f[3]))
        elif f[0] == "scale":
            scales[f[1]] = f[2]
    images = {fn[:-4]: open(os.path.join(out_dir, fn), "rb").read() for fn in sorted(os.listdir(out_dir)) if fn.endswith(".bin") and fn != "blob.bin"}
    return total, sizes, scales, images


@pytest.fixture(scope="module")
def dumped(dump, tmp_path_factory):
    base = tmp_path_factory.mktemp("wimg_out")
    return {name: run_images(dump, name, str(base / name)) for name in CONFIGS}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_images_and_scales_equal_the_goldens(dumped, name):
    golden = json.load(open(GOLDEN))[name]
    total, _, scales, images = dumped[name]
    assert total == golden["total"]
    assert sorted(images) == sorted(golden["images"]), "the set of images this load builds changed"
    for k, data in images.items():
        assert hashlib.sha256(data).hexdigest() == golden["images"][k], f"image {k} of {name} changed"
    assert len(scales) == 6 and scales == golden["scales"]
    for k, v in scales.items():
        assert float.fromhex(v) == float.fromhex(golden["scales"][k])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_image_has_the_size_the_handle_allocates(dumped, name):
    _, sizes, _, images = dumped[name]
    assert set(images) <= set(sizes), "an image was built that the handle does not allocate"
    for k, data in images.items():
        elem, count = sizes[k]
        assert len(data) == elem * count, (k, len(data), elem, count)
    rnn, enc, dec = CONFIGS[name][:3]
    family = {"WmemT", "gUa", "gWcatT"} if rnn == "bigru" else {"WmemT", "Up", "Ua", "WcatT", "Wmp", "Wmp16", "Wkp16"}
    assert family <= set(images)
    assert (("gWx16" if rnn == "bigru" else "Wx16") in sizes) == (enc > 1)
    assert ("W1c16" in sizes) == (rnn == "bilstm" and dec == 2)
    assert ("Wc16" in images) == (rnn == "bilstm" and dec <= 2)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_blob_walk_equals_weights_py(dumped, name):
    from ravvent_basecaller_amd import weights
    assert dumped[name][0] == weights.blob_size(_cfg(name))


@pytest.mark.parametrize("name", ["bilstm-2-1-luong-parts1", "bilstm-3-2-vocab5", "bilstm-1-3"])
def test_rounding_through_the_blob_walk(dump, tmp_path, name):
    from ravvent_basecaller_amd import weights
    from test_weight_parts import numpy_rounded_view
    cfg, flat = make_flat(name)
    src, dst = str(tmp_path / "blob.bin"), str(tmp_path / "rounded.bin")
    weights.pack(cfg, flat).tofile(src)
    subprocess.run([dump, "round", src, dst, str(cfg.enc_depth), str(cfg.dec_depth), str(cfg.vocab)], check=True)
    got = weights.unpack(cfg, np.fromfile(dst, np.float32))
    want = numpy_rounded_view(flat)
    for k in want:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


# ---------------------------------------------------------------- the shared fragment writer, against the documented layouts
def column_scales(mx):
    """The power of two that brings each largest |w| into [2^13, 2^14); 2^14 for a zero one (split_image.h: rv_column_scale)."""
    _, ex = np.frexp(mx)
    return np.ldexp(np.float32(1), 14 - np.where(mx > 0, ex, 0)).astype(np.float32)


def two_parts(v, lo_mul=1.0):
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(lo_mul)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def numpy_recurrent(Uk, g):
    """[8 waves][g gates][4 k-steps][2 parts][64 lanes][8] + 128 g factors: lane (m, kq) of wave w, gate gg, k-step ks holds
    s_r U[32 ks + 8 kq + j][r], r = 128 gg + 16 w + m."""
    Uk = np.asarray(Uk, np.float32)
    assert Uk.shape == (128, 128 * g)
    sc = column_scales(np.abs(Uk).max(axis=0))

    def frag(x):                                                 # [k][r] -> [w][gg][ks][lane = 16 kq + m][j]
        return x.reshape(4, 4, 8, g, 8, 16).transpose(4, 3, 0, 1, 5, 2).reshape(8, g, 4, 64, 8)
    hi, lo = two_parts(Uk * sc)
    img = np.stack([frag(hi), frag(lo)], axis=3)
    return np.concatenate([img.reshape(-1), (np.ldexp(np.float32(1), -14) / sc).astype(np.float32).view(np.uint16)])


def numpy_wq16(Wq):
    """[8 waves][4 k-steps][2 parts][64 lanes][8], one scale: lane (n, kq) of wave wv, k-step ks holds T W_q[32 ks + 8 kq + j][16 wv + n]."""
    Wq = np.asarray(Wq, np.float32)
    T = column_scales(np.abs(Wq).max().reshape(1))[0]

    def frag(x):
        return x.reshape(4, 4, 8, 8, 16).transpose(3, 0, 1, 4, 2).reshape(8, 4, 64, 8)
    hi, lo = two_parts(Wq * T)
    return np.stack([frag(hi), frag(lo)], axis=2).reshape(-1), T


def numpy_wh(W):
    """[32 tiles][2 parts][8 k-steps][64 lanes][8] + 512 factors: lane (n, kq) of tile nt, k-step ks holds s_c W[32 ks + 8 kq + j][16 nt + n];
    part 1 is the f16 rounding of 2048 times what part 0 left."""
    W = np.asarray(W, np.float32)
    assert W.shape == (256, 512)
    sc = column_scales(np.abs(W).max(axis=0))

    def frag(x):
        return x.reshape(8, 4, 8, 32, 16).transpose(3, 0, 1, 4, 2).reshape(32, 8, 64, 8)
    hi, lo = two_parts(W * sc, 2048.0)
    img = np.stack([frag(hi), frag(lo)], axis=1)
    return np.concatenate([img.reshape(-1), (np.ldexp(np.float32(1), -14) / sc).astype(np.float32).view(np.uint16)])


def _pack(exe, tmp_path, kind, mats):
    src, dst = str(tmp_path / f"{kind}.in"), str(tmp_path / f"{kind}.out")
    np.ascontiguousarray(mats, np.float32).tofile(src)
    r = subprocess.run([exe, "pack", kind, src, dst], check=True, capture_output=True, text=True)
    return np.fromfile(dst, np.uint16), r.stdout


def _same(got, want):
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {got.size} uint16 differ, first at {bad[:5]}"


@pytest.mark.parametrize("g", [4, 3])
def test_recurrent_image_matches_documented_layout(dump, tmp_path, g):
    mats = [special_columns(10 + g, 128, 128 * g), (np.random.default_rng(g).standard_normal((128, 128 * g)) * 0.1).astype(np.float32)]
    got, _ = _pack(dump, tmp_path, f"recurrent{g}", np.stack(mats))
    _same(got, np.concatenate([numpy_recurrent(m, g) for m in mats]))


def test_wq16_image_matches_documented_layout(dump, tmp_path):
    rng = np.random.default_rng(5)
    mats = [(rng.standard_normal((128, 128)) * s).astype(np.float32) for s in (0.1, 3e-6, 7e4)] + [np.zeros((128, 128), np.float32)]
    mats[0][17, 99] = np.float32(1.0)                            # the tensor's largest |w| exactly a power of two
    got, out = _pack(dump, tmp_path, "wq16", np.stack(mats))
    want = [numpy_wq16(m) for m in mats]
    _same(got, np.concatenate([w for w, _ in want]))
    assert [float.fromhex(ln.split()[1]) for ln in out.splitlines()] == [float(T) for _, T in want]
    assert want[0][1] == 2.0 ** 13 and want[3][1] == 2.0 ** 14


def test_wh_low_part_carries_2048(dump, tmp_path):
    mats = [special_columns(20, 256, 512), (np.random.default_rng(6).standard_normal((256, 512)) * 0.08).astype(np.float32)]
    got, _ = _pack(dump, tmp_path, "wh", np.stack(mats))
    _same(got, np.concatenate([numpy_wh(m) for m in mats]))
    # ... which is not the low part every other image keeps: where that one is a normal f16, this one is 2048 times it
    v = mats[1] * column_scales(np.abs(mats[1]).max(axis=0))
    lo, lo2 = two_parts(v)[1].view(np.float16).astype(np.float32), two_parts(v, 2048.0)[1].view(np.float16).astype(np.float32)
    normal = np.abs(lo) >= 2.0 ** -14
    assert normal.any() and np.array_equal(lo2[normal], lo[normal] * 2048)


def test_recurrent_image_one_entry_at_a_time(dump, tmp_path):
    """One non-zero weight at (k, r) of a GRU's U [128][384]: exactly its two uint16 slots (and nothing else but column r's factor) differ
    from the image of the zero kernel, at the documented place -- for a k of every (k-step, quarter, j) class and an r of every (gate,
    wave, m) class."""
    g, N = 3, 384
    slot = 2 * 128 * N + 2 * N
    rng = np.random.default_rng(7)
    ks_ = [0, 7, 8, 31, 32, 75, 127]
    rs_ = [0, 15, 16, 127, 128, 200, 255, 256, N - 1]
    cases = [(k, r) for k in ks_ for r in rs_]
    mats = np.zeros((1 + len(cases), 128, N), np.float32)
    for i, (k, r) in enumerate(cases):
        mats[1 + i, k, r] = np.float32(rng.uniform(0.01, 1.0)) * np.float32(1 + 2.0 ** -12)
    got, _ = _pack(dump, tmp_path, "recurrent3", mats)
    got = got.reshape(1 + len(cases), slot)
    zero = got[0]
    assert not zero[:2 * 128 * N].any()
    for i, (k, r) in enumerate(cases):
        img = got[1 + i]
        gg, w, m, ks, kq, j = r // 128, (r % 128) // 16, r % 16, k // 32, (k % 32) // 8, k % 8
        at = ((((w * g + gg) * 4 + ks) * 2 + 0) * 64 + 16 * kq + m) * 8 + j
        diff = np.flatnonzero(img[:2 * 128 * N] != 0)
        assert set(diff) <= {at, at + 512} and at in diff, (k, r, diff, at)
        f, f0 = img[2 * 128 * N:].view(np.float32), zero[2 * 128 * N:].view(np.float32)
        assert set(np.flatnonzero(f != f0)) <= {r}               # (a weight in [0.5, 1) takes the zero column's scale)
        hi, lo = img[at:at + 1].view(np.float16)[0], img[at + 512:at + 513].view(np.float16)[0]
        assert (float(hi) + float(lo)) * float(f[r]) * 2.0 ** 14 == pytest.approx(float(mats[1 + i, k, r]), rel=2.0 ** -22)


if __name__ == "__main__":      # python tests/test_weight_images.py --record <wimg_dump>: write the goldens from that program's output
    import tempfile
    assert sys.argv[1] == "--record"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name_ in CONFIGS:
            total_, _, scales_, images_ = run_images(sys.argv[2], name_, os.path.join(tmp, name_))
            out[name_] = {"total": total_, "scales": scales_, "images": {k: hashlib.sha256(v).hexdigest() for k, v in images_.items()}}
    json.dump(out, open(GOLDEN, "w"), indent=1, sort_keys=True)
    print("wrote", GOLDEN)
