"""The activation helpers every recurrent cell calls (csrc/common.h: rv_tanh, rv_sigmoid -- the encoder's cell updates in
lstm_mx.hip / lstm_rec.hip and every decoder cell in decode.hip), run on the GPU through a small probe kernel
(tests/kernels/act_probe.hip, built by build() as csrc/libravvent_actprobe.so) and held to numpy fp64 on a dense grid: every float
of [2^-26, 1] at a stride, both signs, a linear grid over [-20, 20], and the special values.

rv_tanh must be accurate in RELATIVE terms: a tanh with an absolute error of ~1e-7 (2 sigmoid(2x) - 1, the form before this test and
still the decoder's rv_tanh_abs) is 9e-2 off at |x| ~ 1e-6 and returns 0 below ~3e-8, and a large recurrent gain multiplies that
error at every step (test_bench_config_gpu.test_matrix_pipe_recurrence_adversarial_recurrent_kernel); on that form this test fails
with a relative error of 8.6e-2 at x = -1.04e-6.  rv_sigmoid is pinned against regressions only."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc", "libravvent_actprobe.so")

TANH_REL = 1e-6           # relative error of rv_tanh on 2^-20 <= |x| <= 9
# rv_sigmoid = v_rcp_f32(1 + exp(-x)): measured on MI355X at 9.4e-7 relative on [-16, 16] (worst near x = -14.6, where the rounding
# of x log2(e) carries into exp); bound = that plus a margin of 60 %
SIGMOID_REL = 1.5e-6


def _run_probe(x, path=None):
    import torch  # noqa: F401  (torch's HIP runtime first, as the library's loader does, so that both share one)
    p = path or PROBE
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} not built: run __graft_entry__.build()")
    lib = ctypes.CDLL(p)
    lib.rv_act_probe.restype = ctypes.c_int
    lib.rv_act_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    x = np.ascontiguousarray(x, dtype=np.float32)
    t, s = np.empty_like(x), np.empty_like(x)
    rc = lib.rv_act_probe(x.ctypes.data, t.ctypes.data, s.ctypes.data, x.size)
    assert rc == 0, f"rv_act_probe: hipError {rc}"
    return t, s


def _grid():
    lo, hi = np.float32(2.0 ** -26).view(np.int32), np.float32(1.0).view(np.int32)
    pos = np.concatenate([np.arange(lo, hi + 1, 61, dtype=np.int32).view(np.float32),      # every 61st float of [2^-26, 1]
                          np.linspace(0, 20, 200001, dtype=np.float32)[1:]])               # and [0, 20] at 1e-4
    special = np.array([2.0 ** -20, np.nextafter(np.float32(2.0 ** -20), np.float32(0)), 2.0 ** -126, 1e-45, 3e-8, 1e-5,
                        0.25, np.nextafter(np.float32(0.25), np.float32(0)), np.nextafter(np.float32(0.25), np.float32(1)), 0.3466,
                        9.0, np.nextafter(np.float32(9), np.float32(0)), 16.0, 88.0, 89.0, 104.0, 3.4e38], dtype=np.float32)
    pos = np.concatenate([pos, special])
    return np.concatenate([pos, -pos, np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)])


def test_activation_helpers_against_fp64():
    x = _grid()
    t, s = _run_probe(x)
    x64 = x.astype(np.float64)
    fin = np.isfinite(x)
    ax = np.abs(x64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        t64 = np.tanh(x64)
        s64 = 1.0 / (1.0 + np.exp(-x64))
        rel_t = np.abs(t.astype(np.float64) - t64) / np.abs(t64)
        rel_s = np.abs(s.astype(np.float64) - s64) / s64

    # ---- rv_tanh
    mid = fin & (ax >= 2.0 ** -20) & (ax <= 9.0)
    tiny = fin & (ax < 2.0 ** -20)
    worst_t = float(rel_t[mid].max())
    at = float(x[mid][np.argmax(rel_t[mid])])
    ulps = np.abs(t[tiny].astype(np.float64) - x64[tiny]) / np.spacing(np.abs(x[tiny])).astype(np.float64)
    print(f"rv_tanh: max relative error {worst_t:.3e} (at x = {at:.6g}) on 2^-20 <= |x| <= 9; "
          f"max |t - x| / ulp(x) below 2^-20: {float(ulps.max()):.2f}")
    assert worst_t <= TANH_REL, f"rv_tanh relative error {worst_t:.3e} at x = {at!r} > {TANH_REL}"
    assert (ulps <= 1.0).all(), "rv_tanh(x) is more than one ulp from x below 2^-20"
    n = (x.size - 5) // 2                                       # the grid is [pos, -pos, 5 specials]
    assert np.array_equal(x[:n], -x[n:2 * n])
    assert np.array_equal(t[:n].view(np.int32), (-t[n:2 * n]).view(np.int32)), "rv_tanh is not exactly odd"
    assert (np.abs(t[~np.isnan(x)]) <= 1.0).all(), "|rv_tanh| > 1"
    big = fin & (ax >= 9.0)
    assert (t[big] == np.sign(x[big])).all(), "rv_tanh is not exactly +-1 for |x| >= 9"
    sp = t[-5:]                                                  # +0, -0, +inf, -inf, NaN
    assert sp[0] == 0.0 and not np.signbit(sp[0]) and sp[1] == 0.0 and np.signbit(sp[1]), "rv_tanh(+-0) != +-0"
    assert sp[2] == 1.0 and sp[3] == -1.0, "rv_tanh(+-inf) != +-1"
    assert np.isnan(sp[4]), "rv_tanh(NaN) is not NaN"

    # ---- rv_sigmoid
    box = fin & (ax <= 16.0)
    worst_s = float(rel_s[box].max())
    print(f"rv_sigmoid: max relative error {worst_s:.3e} (at x = {float(x[box][np.argmax(rel_s[box])]):.6g}) on [-16, 16]")
    assert worst_s <= SIGMOID_REL, f"rv_sigmoid relative error {worst_s:.3e} > {SIGMOID_REL}"
    assert ((s[~np.isnan(x)] >= 0.0) & (s[~np.isnan(x)] <= 1.0)).all(), "rv_sigmoid outside [0, 1]"
    assert s[-3] == 1.0 and s[-2] == 0.0 and np.isnan(s[-1]), "rv_sigmoid(+inf, -inf, NaN) != (1, 0, NaN)"
