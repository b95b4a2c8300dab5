"""The activation helpers every recurrent cell calls (csrc/common.h: rv_tanh, rv_sigmoid -- the encoder's cell updates in
lstm_mx.hip / lstm_rec.hip and every decoder cell in decode.hip -- and rv_tanh_abs, the g gate of one decode form), run on the GPU through a small probe kernel
(tests/kernels/act_probe.hip, built by build() as csrc/libravvent_actprobe.so) and held to numpy fp64 on a dense grid: every float
of [2^-26, 1] at a stride, both signs, a linear grid over [-20, 20], and the special values.

rv_tanh must be accurate in RELATIVE terms: a tanh with an absolute error of ~1e-7 (2 sigmoid(2x) - 1, the form before this test and
still the decoder's rv_tanh_abs) is 9e-2 off at |x| ~ 1e-6 and returns 0 below ~3e-8, and a large recurrent gain multiplies that
error at every step (test_bench_config_gpu.test_matrix_pipe_recurrence_adversarial_recurrent_kernel); on that form this test fails
with a relative error of 8.6e-2 at x = -1.04e-6.  rv_sigmoid is pinned against regressions only.

rv_tanh_abs is that absolute form, kept for ONE site: the g gate of k_dec_persist<.., ATT = 2> (decode.hip, dec_gate_tanh).  It is held
to what its formula can give in fp32, and the test also asserts the property that keeps it out of every other site."""
import ctypes
import os

import numpy as np
import pytest

from test_bench_config_gpu import TWIN_K

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


def _run_tanh_abs_probe(x, path=None):
    import torch  # noqa: F401  (as in _run_probe)
    p = path or PROBE
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} not built: run __graft_entry__.build()")
    lib = ctypes.CDLL(p)
    lib.rv_act_probe_tanh_abs.restype = ctypes.c_int
    lib.rv_act_probe_tanh_abs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    x = np.ascontiguousarray(x, dtype=np.float32)
    t = np.empty_like(x)
    rc = lib.rv_act_probe_tanh_abs(x.ctypes.data, t.ctypes.data, x.size)
    assert rc == 0, f"rv_act_probe_tanh_abs: hipError {rc}"
    return t


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


def test_tanh_abs_against_fp64():
    """rv_tanh_abs(x) = 2 / (1 + exp(-2x)) - 1 on the grid of the test above: max |rv_tanh_abs - tanh| over the finite grid no larger
    than TWIN_K x that of a numpy float32 evaluation of the same formula plus one ulp of 1.0 (both maxima over the same points, as the
    tensors' twin-relative bound takes them; the ulp is the spacing of the values the formula's last subtraction produces);
    |rv_tanh_abs| <= 1, +-1 at +-inf, NaN at NaN.

    Why no recurrence may use it: the formula's error is ABSOLUTE, about one ulp of 1.0, whatever |x| -- at |x| = 1e-6 its result
    moves in steps of 1.2e-7 and is wrong by several per cent, where rv_tanh holds TANH_REL.  A recurrent gain multiplies such an
    error step after step (test_bench_config_gpu.test_decoder_adversarial_recurrent_kernel).  The last assertion states that property:
    if it ever fails the helper has become relatively accurate, and its one site and this docstring want revisiting."""
    x = np.concatenate([_grid(), np.array([1e-6, -1e-6], dtype=np.float32)])
    t = _run_tanh_abs_probe(x)
    x64 = x.astype(np.float64)
    fin = np.isfinite(x)
    t64 = np.tanh(x64)
    with np.errstate(over="ignore", invalid="ignore"):
        t32 = np.float32(2.0) / (np.float32(1.0) + np.exp(np.float32(-2.0) * x)) - np.float32(1.0)
    assert t32.dtype == np.float32
    err = np.abs(t[fin].astype(np.float64) - t64[fin])
    err32 = np.abs(t32[fin].astype(np.float64) - t64[fin])
    ulp1 = float(np.spacing(np.float32(1.0)))
    worst, worst32 = float(err.max()), float(err32.max())
    print(f"rv_tanh_abs: max |t - tanh| {worst:.3e} (at x = {float(x[fin][np.argmax(err)]):.6g}); numpy float32 formula {worst32:.3e}; "
          f"ratio {worst / worst32:.2f}")
    assert worst <= TWIN_K * worst32 + ulp1, f"rv_tanh_abs absolute error {worst:.3e} > {TWIN_K} x {worst32:.3e} + {ulp1:.3e}"
    assert (np.abs(t[~np.isnan(x)]) <= 1.0).all(), "|rv_tanh_abs| > 1"
    sp = t[-7:-2]                                                # +0, -0, +inf, -inf, NaN
    assert sp[2] == 1.0 and sp[3] == -1.0, "rv_tanh_abs(+-inf) != +-1"
    assert np.isnan(sp[4]), "rv_tanh_abs(NaN) is not NaN"
    assert np.isinf(x[-5]) and np.isinf(x[-4]) and np.isnan(x[-3])
    small = t[-2:].astype(np.float64)                            # x = 1e-6, -1e-6
    rel = np.abs(small - t64[-2:]) / np.abs(t64[-2:])
    print(f"rv_tanh_abs: relative error at x = +-1e-6: {rel[0]:.3e}, {rel[1]:.3e} (rv_tanh is held to {TANH_REL})")
    assert (rel > TANH_REL).all(), f"rv_tanh_abs is relatively accurate at |x| = 1e-6 ({rel}): see the docstring"
