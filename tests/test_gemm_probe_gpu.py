"""The three projection GEMM kernels of csrc/gemm_f32.hip, each on its own, fed chosen A, W, bias and M through a probe
(tests/kernels/gemm_probe.hip, built by build() as csrc/libravvent_gemmprobe.so) and held to numpy fp64:

  k_gemm_f32<2,2,16>   through launch_gemm_f32 with the library's three argument sets: "keys" (N = 128, row mask, plain grid),
                       "memory" (N = 256, xcd_remap) and "inproj" (N = 512, both directions as two problems, biases, ldc = 1024, xcd_remap);
  k_gemm_mem_split3<1> through launch_gemm_split_blocks with ncb = 1 ("split1": the default attention-memory projection);
  k_gemm_ws            through launch_gemm_split_blocks with ncb = 4 ("ws": the default input projection of encoder layers >= 1)
                       and with ncb = 3 ("ws3": N = 768, the input projection of a BiGRU layer >= 1 -- six half column blocks, so the
                       workgroup id is taken modulo a non-power of two, and up to five row-group multiples where ncb = 4 has four).

Reference and bound.  ref = A64 @ W64 + b in fp64; the fp32 chain twin is the k-ordered chain the kernel file's header says the
f32 kernel is: acc = fl32(acc + a_k w_k), k = 0..255 (product and sum in fp64, rounded once per step), + b rounded once more.  The
error of an element is |x - ref| / s_j with s_j = sum_k |w_kj| + |b_j|: against the column's scale with A at its stated bound of 1.
A column with s_j = 0 must come out exactly 0.  Everywhere max gpu <= TWIN_K x max twin over the same elements, no additive term --
except the classes of A named in SPLIT_TERM_CLASSES on the split kernels, which get the derived term SPLIT_TERM (see there).

Rows.  A[r] = base[r % NBASE]: reference and twin exist for the NBASE base rows only, every row of C is held to the first row with
the same base row BIT FOR BIT (a row's arithmetic does not depend on the tile, wave or lane that ran it), and those first rows to
the reference.  The row counts come from the launchers' arithmetic, restated below.  The probe surrounds C with guard rows and, where
ldc > N, guard columns, all prefilled with one NaN pattern: the guards must keep it and no element of [M, N] may.  For "ws3" this is
what shows that each of the six 128-column halves of C is written by some workgroup and that none of them lands outside [M, 768]: a
half skipped or taken twice by `ch = (id >> 3) % nch` leaves the pattern in its columns (run_kernel)."""
import ctypes
import os

import numpy as np
import pytest

from test_bench_config_gpu import TWIN_K
from test_split_image import special_weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc", "libravvent_gemmprobe.so")

K = 256
NBASE = 509                       # distinct base rows (a prime: every tile, wave and lane position meets every residue)
NWIDE = 1024                      # the references are computed once, 1024 columns wide; a kernel with N columns uses the first N
FILL = 0x7FC5A5A5                 # the prefill of C: a NaN no arithmetic produces
# Split kernels only: a' . w' = ah.wh + ah.wl + al.wh drops al.wl, and each operand's second part is itself rounded: three terms of at
# most 2^-22 |a w| each, so 3 x 2^-22 in the metric above.  Granted to the classes of A whose twin error is far below what the split
# form can give relative to the column's scale (rows scaled by 2^-20 and 2^-30 put 2^14 a into the f16 subnormals, where the parts
# keep fewer bits; a one-hot row leaves the twin exact, so any error at all exceeds TWIN_K x 0); measured ratios: DESIGN.md section 5.
SPLIT_TERM = 3 * 2.0 ** -22
SPLIT_TERM_CLASSES = ("scale20", "scale30", "onehot")

KERNELS = ("keys", "memory", "inproj", "split1", "ws", "ws3")
NCOLS = {"keys": 128, "memory": 256, "inproj": 1024, "split1": 256, "ws": 1024, "ws3": 768}
IS_SPLIT = {"keys": False, "memory": False, "inproj": False, "split1": True, "ws": True, "ws3": True}
WS_NCB = {"ws": 4, "ws3": 3}      # column blocks of the two k_gemm_ws entries


# ---------------------------------------------------------------- the launchers' arithmetic (csrc/gemm_f32.hip), restated
def ws_geometry(M, ncb=4):
    """launch_gemm_split_blocks, ncb = 4 or 3 -> k_gemm_ws: (k, ntile, tiles of the busiest wave).  ncb = 4: eight half column blocks,
    k starts at 256 / 64 = 4; ncb = 3: six, k starts at 256 / 48 = 5."""
    nch, nw = 2 * ncb, 768 // 64
    ntile = (M + 31) // 32
    k = 256 // (8 * nch)
    while k > 1 and 8 * (k - 1) * nw >= ntile:
        k -= 1
    tstride = nw * 8 * k                                   # a wave's tiles: rg + nrg (wave + 12 j) < ntile
    return k, ntile, (ntile + tstride - 1) // tstride


def _ws_rows(ncb=4):
    geo = lambda m: ws_geometry(m, ncb)
    small = [1, 8, 9, 31, 32, 33, 32 * 8 - 1, 32 * 8 + 1]                       # ... ntile 8 and 9
    assert [geo(m)[1] for m in small[-2:]] == [8, 9]
    edges = []
    kmax = geo(1 << 20)[0]
    assert kmax == {4: 4, 3: 5}[ncb]                                            # ncb = 3 reaches a row-group multiple ncb = 4 never does
    for k in range(1, kmax):                                                    # the largest M that still selects k row-group multiples
        m = max(m for m in range(32, 1 << 15, 32) if geo(m)[0] == k)
        assert geo(m + 1)[0] == k + 1
        edges.append(m)
    m = max(m for m in range(32, 1 << 16, 32) if geo(m)[2] == 1)                # the largest M without a second tile per wave
    assert geo(m) == (kmax, 96 * kmax, 1) and geo(m + 1)[2] == 2
    edges.append(m)
    large = []
    for m in edges:                                                             # M % 32 == 0, in 1..8 (past the edge), in 9..31 (before it)
        large += [m - 15, m, m + 1]
    m3 = min(m for m in range(32, 1 << 16, 32) if geo(m + 1)[2] == 3)           # ... and past a third tile: the three residues again
    large += [m3 + 1, m3 + 32 + 20, m3 + 64]
    assert all(geo(m)[2] == 3 for m in large[-3:])
    assert {m % 32 == 0 for m in large} == {True, False} and any(1 <= m % 32 <= 8 for m in large) and any(m % 32 >= 9 for m in large)
    return small + large


def _split1_rows():
    tile, grid = 128, 256               # k_gemm_mem_split3: 128-row tiles, at most 256 workgroups, workgroup w takes tiles w, w + 256, ...
    return [1, tile - 1, tile, tile + 1, grid * tile, grid * tile + 1, grid * tile + 3 * tile + 5, 2 * grid * tile + 77]


def _f32_rows():
    bm, pad = 128, 8                    # k_gemm_f32<2,2,16>: 128-row tiles; xcd_remap pads the row tiles to a multiple of 8
    return [1, bm - 1, bm, bm + 1, pad * bm, pad * bm + 1, 3 * pad * bm + 1]


ROW_CASES = ([("ws", m) for m in _ws_rows(4)] + [("ws3", m) for m in _ws_rows(3)] + [("split1", m) for m in _split1_rows()]
             + [(kern, m) for kern in ("keys", "memory", "inproj") for m in _f32_rows()])


# ---------------------------------------------------------------- probe
_lib = None


def _probe():
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (torch's HIP runtime first, as the library's loader does, so that both share one)
        if not os.path.exists(PROBE):
            raise FileNotFoundError(f"{PROBE} not built: run __graft_entry__.build()")
        lib = ctypes.CDLL(PROBE)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        lib.rv_gemm_probe_guard_rows.restype = ci
        lib.rv_gemm_probe_f32.restype = ci
        lib.rv_gemm_probe_f32.argtypes = [ci, vp, ci, vp, vp, vp, vp, vp, ctypes.c_uint32, vp]
        lib.rv_gemm_probe_split.restype = ci
        lib.rv_gemm_probe_split.argtypes = [ci, vp, ci, vp, vp, ci, ctypes.c_uint32, vp]
        _lib = lib
    return _lib


def _ptr(x):
    return None if x is None else x.ctypes.data


def run_kernel(kern, A, W, bias, mask=None, guard_cols=0):
    """C with its guard rows (and guard columns), [M + guard][ldc], as the kernel left it.  W [256][>= N], bias [>= N] or None."""
    lib = _probe()
    N = NCOLS[kern]
    A = np.ascontiguousarray(A, dtype=np.float32)
    M = A.shape[0]
    assert A.shape == (M, K)
    G = lib.rv_gemm_probe_guard_rows()
    if IS_SPLIT[kern]:
        ldc = N + guard_cols
        Wc = np.ascontiguousarray(W[:, :N], dtype=np.float32)
        b = None if bias is None else np.ascontiguousarray(bias[:N], dtype=np.float32)
        C = np.empty((M + G, ldc), dtype=np.float32)
        rc = lib.rv_gemm_probe_split(N // 256, A.ctypes.data, M, Wc.ctypes.data, _ptr(b), ldc, FILL, C.ctypes.data)
    else:
        assert guard_cols == 0
        which = KERNELS.index(kern)
        if kern == "inproj":
            W0, W1 = (np.ascontiguousarray(W[:, i:i + 512], dtype=np.float32) for i in (0, 512))
            b0, b1 = (np.ascontiguousarray(bias[i:i + 512], dtype=np.float32) for i in (0, 512))
        else:
            assert bias is None
            W0, W1, b0, b1 = np.ascontiguousarray(W[:, :N], dtype=np.float32), None, None, None
        m8 = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        C = np.empty((M + G, N), dtype=np.float32)
        rc = lib.rv_gemm_probe_f32(which, A.ctypes.data, M, W0.ctypes.data, _ptr(W1), _ptr(b0), _ptr(b1), _ptr(m8), FILL, C.ctypes.data)
    assert rc == 0, f"gemm probe ({kern}, M = {M}): hipError {rc}"
    bits = C.view(np.uint32)
    assert (bits[M:] == FILL).all(), f"{kern}, M = {M}: a guard row was written"
    assert (bits[:, N:] == FILL).all(), f"{kern}, M = {M}: a guard column was written"
    inside = bits[:M, :N] == FILL
    # (relied on for "ws3", nch = 6: every one of the six 128-column halves written, by whichever workgroup `% nch` gives it to)
    assert not inside.any(), f"{kern}, M = {M}: {int(inside.sum())} elements never written, first at {np.argwhere(inside)[:4].tolist()}"
    return C[:M, :N]


# ---------------------------------------------------------------- operands, fp64 reference, fp32 chain twin
def _weights(kind):
    rng = np.random.default_rng(11 if kind == "ordinary" else 12)
    return (rng.standard_normal((K, NWIDE)) * 0.08).astype(np.float32) if kind == "ordinary" else special_weights(rng, NWIDE)


def _bias(W, kind):
    """None, an ordinary bias, or one 1e3 x the size of the product (the rms of a . w_j for uniform a); 0 for a zero column either way."""
    if kind == "none":
        return None
    rng = np.random.default_rng(13)
    rms = np.sqrt((W.astype(np.float64) ** 2).sum(axis=0) / 3.0)
    sgn = rng.choice([-1.0, 1.0], NWIDE)
    return (sgn * rms * (rng.uniform(0.2, 1.0, NWIDE) if kind == "ordinary" else 1e3)).astype(np.float32)


def _base_rows():
    rng = np.random.default_rng(14)
    return rng.uniform(-1.0, 1.0, (NBASE, K)).astype(np.float32)


VALUE_CLASSES = ("uniform", "edge", "scale10", "scale20", "scale30", "zero", "onehot")


def _value_rows():
    """(A, class of each row): uniform(-1, 1); +-1.0 and nextafter(1, 0) among ordinary values; rows scaled by 2^-10, 2^-20, 2^-30;
    zero rows, -0.0 rows and ordinary rows with -0.0 entries; the 256 one-hot rows (row 'onehot' i = e_i)."""
    rng = np.random.default_rng(15)
    parts, cls = [], []

    def add(name, rows):
        parts.append(rows.astype(np.float32)); cls.extend([name] * len(rows))
    add("uniform", rng.uniform(-1, 1, (69, K)))
    e = rng.uniform(-1, 1, (64, K)).astype(np.float32)
    pick = rng.uniform(size=e.shape)
    e[pick < 0.1] = 1.0; e[(pick >= 0.1) & (pick < 0.2)] = -1.0
    e[(pick >= 0.2) & (pick < 0.3)] = np.nextafter(np.float32(1), np.float32(0)); e[(pick >= 0.3) & (pick < 0.4)] = -np.nextafter(np.float32(1), np.float32(0))
    e[0, :] = 1.0; e[1, :] = -1.0; e[2, :] = np.nextafter(np.float32(1), np.float32(0))
    add("edge", e)
    for p in (10, 20, 30):
        add(f"scale{p}", rng.uniform(-1, 1, (32, K)) * 2.0 ** -p)
    z = np.zeros((8, K), dtype=np.float32)
    z[2:4] = -0.0
    z[4:] = rng.uniform(-1, 1, (4, K)); z[4:][rng.uniform(size=(4, K)) < 0.5] = -0.0
    add("zero", z)
    add("onehot", np.eye(K))
    A = np.concatenate(parts)
    return A, np.array(cls)


def _chain(A, W):
    """(fp64 product, fp32 chain twin before the bias) of A [m][256] and W [256][n]."""
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    acc = np.zeros((A.shape[0], W.shape[1]), dtype=np.float32)
    for k in range(K):
        acc = (acc.astype(np.float64) + A64[:, k, None] * W64[None, k, :]).astype(np.float32)
    return A64 @ W64, acc


_cache = {}


def _reference(rows, wkind):
    """Shared and left unchanged: (A, classes or None, W, fp64 product, twin accumulator) of the base rows / the value rows x a W."""
    key = (rows, wkind)
    if key not in _cache:
        if ("A", rows) not in _cache:
            _cache[("A", rows)] = (_base_rows(), None) if rows == "base" else _value_rows()
        A, cls = _cache[("A", rows)]
        W = _weights(wkind)
        ref, acc = _chain(A, W)
        for x in (A, W, ref, acc):
            x.setflags(write=False)
        _cache[key] = (A, cls, W, ref, acc)
    return _cache[key]


def _with_bias(W, ref, acc, bias):
    """(ref, twin, s): the bias added (the twin's rounded once more) and the columns' scales."""
    s = np.abs(W.astype(np.float64)).sum(axis=0)
    if bias is None:
        return ref, acc, s
    b64 = bias.astype(np.float64)
    return ref + b64, (acc.astype(np.float64) + b64).astype(np.float32), s + np.abs(b64)


def _errors(x, ref, s):
    """max over the elements of |x - ref| / s_j; columns with s_j = 0 must be exactly 0 and do not enter."""
    live = s > 0
    assert (x[:, ~live] == 0).all(), "a column of scale 0 is not exactly 0"
    if x.shape[0] == 0 or not live.any():
        return 0.0
    return float((np.abs(x[:, live].astype(np.float64) - ref[:, live]) / s[live]).max())


def _keys_mask(M, rng):
    """Random, row 0 kept; one whole 128-row tile masked where there is a second one; (mask, a masked row to hold NaN or None)."""
    mask = (rng.uniform(size=M) < 0.75).astype(np.uint8)
    mask[0] = 1
    if M >= 256:
        mask[128:256] = 0
    off = np.flatnonzero(mask == 0)
    return mask, (int(off[len(off) // 2]) if off.size else None)


# ---------------------------------------------------------------- rows
@pytest.mark.parametrize("kern,M", ROW_CASES, ids=[f"{k}-{m}" for k, m in ROW_CASES])
def test_gemm_rows(kern, M):
    """Every row count at which the launch geometry changes (module docstring), uniform A, the special W (column scales 2^+-20, a zero
    column, an outlier entry, column maxima at and just below a power of two), an ordinary bias where the kernel takes one."""
    A0, _, W, ref, acc = _reference("base", "special")
    N = NCOLS[kern]
    bias = None if kern in ("keys", "memory") else _bias(W, "ordinary")
    ref, twin, s = _with_bias(W, ref, acc, bias)
    ref, twin, s = ref[:, :N], twin[:, :N], s[:N]
    base = np.arange(M) % NBASE
    A = A0[base]
    mask, nan_row = None, None
    if kern == "keys":
        mask, nan_row = _keys_mask(M, np.random.default_rng(M))
        if nan_row is not None:
            A[nan_row] = np.nan
    C = run_kernel(kern, A, W, bias, mask=mask, guard_cols=32 if IS_SPLIT[kern] and M % 2 else 0)
    kept = np.arange(M) if mask is None else np.flatnonzero(mask)
    if mask is not None:
        dropped = C[mask == 0].view(np.uint32)
        assert (dropped == 0).all(), f"{kern}, M = {M}: a masked row is not exactly +0 (row {nan_row} of A holds NaN)"
    # every kept row bit for bit the first kept row with its base row
    ub, first, inv = np.unique(base[kept], return_index=True, return_inverse=True)
    T = C[kept[first]]
    same = (C[kept].view(np.uint32) == T.view(np.uint32)[inv]).all(axis=1)
    assert same.all(), f"{kern}, M = {M}: rows {kept[~same][:8].tolist()} differ from the first row with the same A row"
    e_gpu, e_twin = _errors(T, ref[ub], s), _errors(twin[ub], ref[ub], s)
    ident = float((T.view(np.uint32) == twin[ub].view(np.uint32)).mean())
    print(f"gemm rows {kern} M = {M}: gpu {e_gpu:.3e} twin {e_twin:.3e} ratio {e_gpu / e_twin:.3f}"
          + ("" if IS_SPLIT[kern] else f"; bit-identical to the twin: {100 * ident:.2f} %"))
    assert e_gpu <= TWIN_K * e_twin, f"{kern}, M = {M}: {e_gpu:.3e} > {TWIN_K} x {e_twin:.3e}"


# ---------------------------------------------------------------- values
def _value_M(cls):
    """(rows of the small case, M of the ragged case): the small case takes two rows of every class and eight one-hot rows, one tile
    of every kernel; the ragged case all rows, 493 = 3 x 128 + 109 = 15 x 32 + 13."""
    sel = []
    for c in VALUE_CLASSES:
        idx = np.flatnonzero(cls == c)
        sel += list(idx[:2]) if c != "onehot" else [int(idx[k]) for k in (0, 7, 8, 31, 32, 128, 254, 255)]
    return np.array(sel), len(cls)


@pytest.mark.parametrize("wkind", ["ordinary", "special"])
@pytest.mark.parametrize("kern", KERNELS)
def test_gemm_values(kern, wkind):
    """The classes of A (VALUE_CLASSES) x an ordinary and the special W x no bias, an ordinary one and one 1e3 x the product (where the
    kernel takes one), at one small and one ragged M: per class (small M: per group of classes with one bound) max gpu <= TWIN_K x
    max twin (+ SPLIT_TERM on SPLIT_TERM_CLASSES of a split kernel), and the one-hot rows return their row of W: W[k, :] + b exactly on the f32 kernel; within 2^-22 |w| + ulp on the
    split kernels, ulp = the f32 spacing of the larger of |w| and |w + b| -- and, only where s_c |w| < 2^-3 so that the weight's
    second f16 part is a subnormal of spacing 2^-24, 2^-25 / s_c more.  This holds the image's k and column order one entry at a time."""
    A, cls, W, ref0, acc0 = _reference("values", wkind)
    N = NCOLS[kern]
    sel, Mfull = _value_M(cls)
    biases = ["none"] if kern in ("keys", "memory") else (["ordinary", "big"] if kern == "inproj" else ["none", "ordinary", "big"])
    failures = []
    for bkind in biases:
        bias = _bias(W, bkind)
        ref, twin, s = _with_bias(W, ref0, acc0, bias)
        ref, twin, s = ref[:, :N], twin[:, :N], s[:N]
        for rows in (sel, np.arange(Mfull)):
            mask = np.ones(len(rows), dtype=np.uint8) if kern == "keys" else None
            C = run_kernel(kern, A[rows], W, bias, mask=mask, guard_cols=64 if IS_SPLIT[kern] and len(rows) == Mfull else 0)
            # the ragged case holds every class on its own; the small one has two rows of a class -- 256 elements of a column-sparse
            # maximum -- so there the classes that share a bound are held together (each class's figures are still printed)
            plain = tuple(c for c in VALUE_CLASSES if c not in SPLIT_TERM_CLASSES)
            groups = [(c,) for c in VALUE_CLASSES] if len(rows) == Mfull else [plain, SPLIT_TERM_CLASSES]
            for c in VALUE_CLASSES if len(rows) != Mfull else ():
                at = np.flatnonzero(cls[rows] == c)
                e_gpu, e_twin = _errors(C[at], ref[rows[at]], s), _errors(twin[rows[at]], ref[rows[at]], s)
                print(f"gemm values {kern} W {wkind} bias {bkind} M = {len(rows)} ({c}: gpu {e_gpu:.3e} twin {e_twin:.3e})")
            for g in groups:
                at = np.flatnonzero(np.isin(cls[rows], g))
                e_gpu, e_twin = _errors(C[at], ref[rows[at]], s), _errors(twin[rows[at]], ref[rows[at]], s)
                term = SPLIT_TERM if IS_SPLIT[kern] and g[0] in SPLIT_TERM_CLASSES else 0.0
                ok = e_gpu <= TWIN_K * e_twin + term
                print(f"gemm values {kern} W {wkind} bias {bkind} M = {len(rows)} {'+'.join(g)}: gpu {e_gpu:.3e} twin {e_twin:.3e} ratio "
                      f"{e_gpu / e_twin if e_twin else float('inf') if e_gpu else 0.0:.3f}{'' if ok else '  <-- FAILS'}")
                if not ok:
                    failures.append((bkind, len(rows), g, e_gpu, e_twin))
            # one-hot rows: the row of W they select
            at = np.flatnonzero(cls[rows] == "onehot")
            ks = rows[at] - int(np.flatnonzero(cls == "onehot")[0])
            w = W[ks, :N]
            want = w if bias is None else (w.astype(np.float64) + bias[:N].astype(np.float64)).astype(np.float32)
            if not IS_SPLIT[kern]:
                bad = C[at] != want
                print(f"gemm values {kern} W {wkind} bias {bkind} M = {len(rows)}: one-hot rows exact: {not bad.any()}")
                if bad.any():
                    failures.append((bkind, len(rows), "onehot exact", int(bad.sum()), np.argwhere(bad)[:4].tolist()))
            else:
                mx = np.abs(W[:, :N]).max(axis=0).astype(np.float64)
                sc = 2.0 ** (14 - np.where(mx > 0, np.frexp(mx)[1], 0))
                aw = np.abs(w.astype(np.float64))
                tol = 2.0 ** -22 * aw + np.spacing(np.maximum(np.abs(w), np.abs(want))).astype(np.float64)
                sub = aw * sc < 2.0 ** -3
                tol0, tol = tol, tol + np.where(sub, 2.0 ** -25 / sc, 0.0)
                exact = w.astype(np.float64) + (0.0 if bias is None else bias[:N].astype(np.float64))
                d = np.abs(C[at].astype(np.float64) - exact)
                print(f"gemm values {kern} W {wkind} bias {bkind} M = {len(rows)}: one-hot rows max |x - (w + b)| / tol {float((d / tol).max()):.3f}"
                      f" ({int(sub.sum())} of {sub.size} entries with a subnormal second part, max there {float((d / tol)[sub].max()) if sub.any() else 0.0:.3f},"
                      f" without their term {float((d / tol0)[sub].max()) if sub.any() else 0.0:.3f})")
                if (d > tol).any():
                    failures.append((bkind, len(rows), "onehot tol", int((d > tol).sum()), np.argwhere(d > tol)[:4].tolist()))
    assert not failures, failures


# ---------------------------------------------------------------- non-finite rows
@pytest.mark.parametrize("kern", KERNELS)
def test_gemm_nonfinite_rows_stay_in_their_rows(kern):
    """One NaN row and one +inf row in A: those rows of C are non-finite throughout, every other row is bit for bit the row of the same
    run with the two rows zeroed."""
    A0, _, W, _, _ = _reference("base", "special")
    M = 301                                                  # 2 x 128 + 45 = 9 x 32 + 13
    bias = None if kern in ("keys", "memory") else _bias(W, "ordinary")
    mask = np.ones(M, dtype=np.uint8) if kern == "keys" else None
    A = A0[:M].copy()
    r_nan, r_inf = 37, 270                                   # (k_gemm_ws's paired store: row 37 is an r1, row 270 = 8 x 32 + 14 an r1 + 8)
    A[[r_nan, r_inf]] = 0.0
    clean = run_kernel(kern, A, W, bias, mask=mask)
    A[r_nan] = np.nan
    A[r_inf] = np.inf
    C = run_kernel(kern, A, W, bias, mask=mask)
    assert not np.isfinite(C[[r_nan, r_inf]]).any(), f"{kern}: a NaN / inf row of A left finite elements in its row of C"
    others = np.setdiff1d(np.arange(M), [r_nan, r_inf])
    same = (C[others].view(np.uint32) == clean[others].view(np.uint32)).all(axis=1)
    assert same.all(), f"{kern}: rows {others[~same][:8].tolist()} changed when rows {r_nan} and {r_inf} of A became NaN / inf"
