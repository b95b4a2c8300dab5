"""The split-f16 weight image of the split GEMMs (csrc/split_image.h: rv_pack_split_image, the one packer behind both images
rv_load_weights uploads and behind the kernels' probe), held byte for byte to a numpy restatement of the layout csrc/common.h
documents: [ncb][8 k-steps][16 tiles][2 parts][64 lanes][8 f16] of the column-scaled kernel, then 256 ncb floats 2^-14 / s_c.
Host code only: the packer is reached through the probe library (tests/kernels/gemm_probe.hip: rv_gemm_probe_pack), no GPU needed."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc", "libravvent_gemmprobe.so")


def _pack(W, ncb, ld=None):
    import torch  # noqa: F401  (torch's HIP runtime first, as the library's loader does, so that both share one)
    if not os.path.exists(PROBE):
        raise FileNotFoundError(f"{PROBE} not built: run __graft_entry__.build()")
    lib = ctypes.CDLL(PROBE)
    lib.rv_gemm_probe_pack.restype = ctypes.c_int
    lib.rv_gemm_probe_pack.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    N = 256 * ncb
    ld = ld or N
    buf = np.full((256, ld), np.nan, dtype=np.float32)          # columns past N: never read
    buf[:, :N] = W
    img = np.zeros(2 * 256 * N + 2 * N, dtype=np.uint16)
    assert lib.rv_gemm_probe_pack(buf.ctypes.data, ld, ncb, img.ctypes.data) == 0
    return img


def numpy_image(W, ncb):
    """The documented layout, restated: column c = 256 cb + 16 nt + n; lane (n, kq = lane // 16) of tile nt, k-step ks holds
    s_c W[32 ks + 8 kq + j][c], j = 0..7; part 0 = its f16 rounding, part 1 = the f16 rounding of the rest; s_c = the power of two
    that brings the column's largest |w| into [2^13, 2^14) (2^14 for a zero column); then the factors 2^-14 / s_c as floats."""
    W = np.asarray(W, dtype=np.float32)
    assert W.shape == (256, 256 * ncb)
    mx = np.abs(W).max(axis=0)
    _, ex = np.frexp(mx)                                         # mx = m 2^ex, m in [0.5, 1)
    ex = np.where(mx > 0, ex, 0)
    sc = np.ldexp(np.float32(1), 14 - ex).astype(np.float32)
    v = W * sc                                                   # exact
    assert v.dtype == np.float32 and np.array_equal(v.astype(np.float64), W.astype(np.float64) * sc.astype(np.float64))
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)

    def frag(x):                                                 # [k][c] -> [cb][ks][nt][lane = 16 kq + n][j]
        return x.view(np.uint16).reshape(8, 4, 8, ncb, 16, 16).transpose(3, 0, 4, 1, 5, 2).reshape(ncb, 8, 16, 64, 8)
    img = np.stack([frag(hi), frag(lo)], axis=3)                 # [cb][ks][nt][part][lane][j]
    f = (np.ldexp(np.float32(1), -14) / sc).astype(np.float32)
    return np.concatenate([img.reshape(-1), f.view(np.uint16)])


def special_weights(rng, N):
    """[256][N] weights with, by column c % 16: 3 -> the column x 2^20, 5 -> x 2^-20, 7 -> a zero column, 9 -> one entry x 100,
    11 -> the column's largest |w| exactly a power of two, 13 -> the float just below one; every other column ordinary."""
    W = (rng.standard_normal((256, N)) * 0.08).astype(np.float32)
    c = np.arange(N)
    W[:, c % 16 == 3] *= np.float32(2.0 ** 20)
    W[:, c % 16 == 5] *= np.float32(2.0 ** -20)
    W[:, c % 16 == 7] = 0.0
    for j in c[c % 16 == 9]:
        W[rng.integers(256), j] *= 100.0
    for j in c[(c % 16 == 11) | (c % 16 == 13)]:
        p = np.float32(2.0 ** int(rng.integers(-3, 2)))
        k = int(np.argmax(np.abs(W[:, j])))
        W[:, j] *= np.float32(0.4) * p / np.abs(W[k, j])         # everything else well below p
        W[k, j] = np.copysign(p if j % 16 == 11 else np.nextafter(p, np.float32(0)), W[k, j])
    return W


@pytest.mark.parametrize("ncb", [1, 3, 4])          # the attention memory; both directions of a BiGRU layer; of a BiLSTM layer
@pytest.mark.parametrize("kind", ["ordinary", "special"])
def test_split_image_matches_documented_layout(ncb, kind):
    rng = np.random.default_rng(100 * ncb + len(kind))
    N = 256 * ncb
    W = (rng.standard_normal((256, N)) * 0.08).astype(np.float32) if kind == "ordinary" else special_weights(rng, N)
    want = numpy_image(W, ncb)
    got = _pack(W, ncb)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {got.size} uint16 differ, first at {bad[:5]}"
    if kind == "special":
        # the scales the special columns must get: column maximum s_c in [2^13, 2^14), exactly 2^13 at a power of two
        f = want[2 * 256 * N:].view(np.float32)
        mx = np.abs(W).max(axis=0)
        scaled = mx.astype(np.float64) * 2.0 ** -14 / f
        c = np.arange(N)
        assert (scaled[c % 16 == 11] == 2.0 ** 13).all() and (scaled[c % 16 == 13] == np.nextafter(np.float32(2.0 ** 14), np.float32(0))).all()
        assert (f[c % 16 == 7] == 2.0 ** -28).all() and ((scaled[c % 16 != 7] >= 2.0 ** 13) & (scaled[c % 16 != 7] < 2.0 ** 14)).all()
        # a leading dimension wider than the kernel gives the same bytes
        assert np.array_equal(_pack(W, ncb, ld=N + 24), want)


def test_split_image_one_entry_at_a_time():
    """One non-zero weight at (k, c): exactly its two uint16 slots (and nothing else but column c's factor) differ from the image of
    the zero kernel, at the documented place -- for a k of every (k-step, quarter, j) class and a column of every (block, tile, n) class."""
    ncb = 4
    N = 256 * ncb
    zero = _pack(np.zeros((256, N), dtype=np.float32), ncb)
    assert not zero[:2 * 256 * N].any()
    rng = np.random.default_rng(7)
    ks_ = list(range(0, 256, 37)) + [7, 8, 31, 32, 255]
    cs_ = list(range(0, N, 97)) + [15, 16, 255, 256, N - 1]
    for k in ks_:
        for c in cs_:
            W = np.zeros((256, N), dtype=np.float32)
            W[k, c] = np.float32(rng.uniform(0.01, 1.0)) * np.float32(1 + 2.0 ** -12)
            img = _pack(W, ncb)
            cb, nt, n, ks, kq, j = c // 256, (c % 256) // 16, c % 16, k // 32, (k % 32) // 8, k % 8
            at = ((((cb * 8 + ks) * 16 + nt) * 2 + 0) * 64 + 16 * kq + n) * 8 + j
            diff = np.flatnonzero(img[:2 * 256 * N] != 0)
            assert set(diff) <= {at, at + 512} and at in diff, (k, c, diff, at)
            f = img[2 * 256 * N:].view(np.float32)[c]
            hi, lo = img[at:at + 1].view(np.float16)[0], img[at + 512:at + 513].view(np.float16)[0]
            assert (float(hi) + float(lo)) * float(f) * 2.0 ** 14 == pytest.approx(float(W[k, c]), rel=2.0 ** -22)
