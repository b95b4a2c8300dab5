"""The signals of tests/test_signal_prep_gpu.py, and the host statements they are held to.  tests/test_signal_prep.py proves on the host
alone that each named input contains what it is there for, so that the GPU file never passes on an input that lost its point."""
import numpy as np

# every start-up length of the detector (windows up to 9: the ring holds 19 sums, the start-up ends by sample 2 * 19), both sides of a
# 256-thread workgroup, of the scan's 2048-sample tile and of two tiles, and one read of many tiles
LENGTHS = list(range(0, 71)) + [255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 65537]
MAX_SAMPLES = 1 << 22


def step_signal(n):
    """Integer levels that change every 13 samples, with a 3-sample ripple: events of 10 to 13 samples."""
    k = np.arange(n)
    return (400 + 37 * (((k // 13) * 7) % 11) + (k % 3)).astype(np.int16)


def plateau_signal(n, period=16):
    """+-32767 alternating plateaus: the largest running sums of x^2 a signal of n int16 samples has."""
    k = np.arange(n)
    return np.where((k // period) & 1, 32767, -32767).astype(np.int16)


def flat_signal(n=500):
    return np.full(n, 417, np.int16)


def one_event_signal():
    """Not flat, and short enough to end inside the detector's second event."""
    return step_signal(25)


def synthetic_signal(rv, n_bases, seed):
    sig, _ = rv.synthetic.make_read(n_bases=n_bases, seed=seed)
    return sig


def ordered(x):
    """f32 -> int64 that counts representable values in order: neighbours differ by 1 (and -0.0 sits on +0.0)."""
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def scaled_table_mismatch(got, want):
    """The contract of a scaled table against the host's: every element equal or adjacent in float32, a zero of the host exactly zero,
    at most 1 element in 10,000 different.  -> None, or what is wrong."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float32:
        return f"shape / dtype {got.shape} {got.dtype} against {want.shape}"
    d = np.abs(ordered(got) - ordered(want))
    if d.size and d.max() > 1:
        return f"an element is {int(d.max())} float32 values away"
    if np.any((want == 0) & (got != 0)):
        return "a zero of the host table is not zero"
    n = int(np.count_nonzero(d))
    if n * 10000 > d.size:
        return f"{n} of {d.size} elements differ"
    return None
