"""Stitching a read's chunk calls by signal position: the rule in plain numpy, which the device result equals
bit for bit (tests/test_stitch_gpu.py), and the synthetic reads on which tests/test_stitch.py proves what the rule is good for.

The rule.  A read has chunks k = 0..n-1 in the order of its window rows (raw_start a, raw_len la, event_start e, event_len le).
  position   p[k,i], i < lengths[k]: basecaller.signal_positions (imported, not restated), f64
  ownership  m_k = a_k + 0.5 la_k;  cut_k = 0.5 (m_{k-1} + m_k);  lo_0 = -inf, lo_k = cut_k;  hi_{n-1} = +inf, hi_k = cut_{k+1}
  inside     lo_k <= p[k,i] < hi_k; a NaN is never inside
  kept       i = f_k .. l_k, the first and last inside index of the chunk (the hull); no inside base: nothing
  read       the kept bases of chunk 0, then chunk 1, ...: letter, prob, p, raw_mass, event_mass, source_chunk, source_index"""
import numpy as np

FIELDS = ("bases", "probs", "positions", "raw_mass", "event_mass", "source_chunk", "source_index")
DTYPES = (np.uint8, np.float32, np.float64, np.float32, np.float32, np.int32, np.int32)


def _positions():
    import ravvent_basecaller_amd as rv
    return rv.basecaller.signal_positions


def chunk_positions(mode, windows, lengths, raw_pos, raw_mass, event_pos, event_mass, ev_starts, ev_lengths):
    """p [n, stride] f64 of one read's chunks (windows [n,4]); columns >= lengths[k] (clamped into [0, stride]) are NaN."""
    w = np.asarray(windows, np.int64).reshape(-1, 4)
    n, stride = np.asarray(raw_pos).shape
    p = np.full((n, stride), np.nan, np.float64)
    if n and stride:
        p[:] = _positions()(mode, w[:, 0:1], w[:, 2:3], raw_pos, raw_mass, event_pos, event_mass, ev_starts, ev_lengths)
    ln = np.clip(np.asarray(lengths, np.int64), 0, stride)
    p[np.arange(stride)[None, :] >= ln[:, None]] = np.nan
    return p


def bounds(windows):
    """lo, hi [n] f64 of one read's chunks."""
    w = np.asarray(windows, np.int64).reshape(-1, 4)
    m = w[:, 0].astype(np.float64) + 0.5 * w[:, 1].astype(np.float64)
    cut = 0.5 * (m[:-1] + m[1:])
    return np.concatenate([[-np.inf], cut]), np.concatenate([cut, [np.inf]])


def keep_ranges(p, lo, hi):
    """f [n], count [n] from the positions [n, stride] (NaN beyond a chunk's length) and the bounds: vectorised over the chunks."""
    with np.errstate(invalid="ignore"):
        inside = (lo[:, None] <= p) & (p < hi[:, None])
    n, stride = inside.shape
    if stride == 0:
        return np.zeros(n, np.int64), np.zeros(n, np.int64)
    some = inside.any(axis=1)
    f = np.where(some, inside.argmax(axis=1), 0)
    l = np.where(some, stride - 1 - inside[:, ::-1].argmax(axis=1), -1)
    return f, l - f + 1


def stitch_read(mode, windows, bases, probs, lengths, raw_pos, raw_mass, event_pos, event_mass, ev_starts, ev_lengths):
    """One read -> the seven arrays of FIELDS."""
    n = int(np.asarray(lengths).shape[0])
    if n == 0:
        return tuple(np.zeros(0, dt) for dt in DTYPES)
    p = chunk_positions(mode, windows, lengths, raw_pos, raw_mass, event_pos, event_mass, ev_starts, ev_lengths)
    f, cnt = keep_ranges(p, *bounds(windows))
    col = np.arange(p.shape[1])[None, :]
    kept = (col >= f[:, None]) & (col < (f + cnt)[:, None])          # row-major order = chunk 0's bases, then chunk 1's, ...
    ck, ix = np.nonzero(kept)
    g = lambda a, dt: np.ascontiguousarray(np.asarray(a)[ck, ix], dtype=dt)
    return (g(bases, np.uint8), g(probs, np.float32), g(p, np.float64), g(raw_mass, np.float32), g(event_mass, np.float32),
            ck.astype(np.int32), ix.astype(np.int32))


def stitch(mode, table, read_rows, bases, probs, lengths, raw_pos, raw_mass, event_pos, event_mass, events):
    """Several reads: table [n,5] (read_id first), read_rows [n_reads + 1], events[r] = (starts, lengths) of read r ->
    (the seven arrays of FIELDS concatenated over the reads, read_offsets int64 [n_reads + 1])."""
    table = np.asarray(table, np.int64).reshape(-1, 5)
    parts, offs = [], [0]
    for r in range(len(read_rows) - 1):
        a, b = int(read_rows[r]), int(read_rows[r + 1])
        st, ln = events[r] if events is not None else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        parts.append(stitch_read(mode, table[a:b, 1:], bases[a:b], probs[a:b], lengths[a:b], raw_pos[a:b], raw_mass[a:b], event_pos[a:b],
                                 event_mass[a:b], st, ln))
        offs.append(offs[-1] + len(parts[-1][0]))
    cat = tuple(np.concatenate([p[i] for p in parts]) if parts else np.zeros(0, DTYPES[i]) for i in range(7))
    return cat, np.asarray(offs, np.int64)


def stitch_read_loop(mode, windows, bases, probs, lengths, raw_pos, raw_mass, event_pos, event_mass, ev_starts, ev_lengths):
    """The same rule, base by base in Python: what tests/test_stitch.py holds `stitch_read` to."""
    w = np.asarray(windows, np.int64).reshape(-1, 4)
    n = len(w)
    out = [[] for _ in range(7)]
    pos = _positions()
    for k in range(n):
        m = float(w[k, 0]) + 0.5 * float(w[k, 1])
        lo = -np.inf if k == 0 else 0.5 * ((float(w[k - 1, 0]) + 0.5 * float(w[k - 1, 1])) + m)
        hi = np.inf if k == n - 1 else 0.5 * (m + (float(w[k + 1, 0]) + 0.5 * float(w[k + 1, 1])))
        ln = min(max(int(lengths[k]), 0), np.asarray(raw_pos).shape[1])
        p = [float(pos(mode, w[k, 0], w[k, 2], raw_pos[k, i:i + 1], raw_mass[k, i:i + 1], event_pos[k, i:i + 1], event_mass[k, i:i + 1],
                       ev_starts, ev_lengths)[0]) for i in range(ln)]
        ins = [i for i in range(ln) if lo <= p[i] < hi]
        if not ins:
            continue
        for i in range(ins[0], ins[-1] + 1):
            for o, v in zip(out, (bases[k, i], probs[k, i], p[i], raw_mass[k, i], event_mass[k, i], k, i)):
                o.append(v)
    return tuple(np.asarray(o, dt) for o, dt in zip(out, DTYPES))


def same_bits(a, b):
    """Equal as bytes, with NaN matching NaN (the rule's own wording: a NaN's payload is nobody's contract)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()


# ---- the synthetic read of the property test: bases with true positions, windows that overlap, calls with shared position noise
def synthetic_read(seed, per_chunk_noise=False):
    """-> dict(truth u8 [n_bases], windows i32 [n,4], bases u8 / probs f32 / raw_pos f32 / raw_mass f32 / event_pos / event_mass [n,S],
    lengths i32 [n]).  Bases sit 5-14 samples apart; windows of 150-300 samples start every 20-79 samples, the last start before
    N - T/2; a chunk's call is the bases inside its window; a reported position is the true one plus one noise value per base,
    |noise| < 2.4, the same in every chunk (per_chunk_noise: drawn again per chunk); letters within 12 samples of a window edge that is
    not the read's own edge are corrupted.  Raw mode: positions are raw_start + raw_pos."""
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(40, 400))
    gaps = rng.integers(5, 15, nb)
    true_pos = np.cumsum(gaps).astype(np.int64)                    # integers: raw_pos = pos - a is exact in f32 with the noise below
    N = int(true_pos[-1]) + int(rng.integers(5, 15))
    T = int(rng.integers(150, 301))
    truth = rng.choice(np.frombuffer(b"ACGT", np.uint8), nb)
    starts = [0]
    while True:
        s = starts[-1] + int(rng.integers(20, 80))
        if s >= N - T / 2:
            break
        starts.append(s)
    noise = rng.integers(-614, 615, nb) / 256.0                   # multiples of 2^-8: raw_start + f32(raw_pos) is the same f64 in every chunk
    rows, calls = [], []
    for k, a in enumerate(starts):
        la = min(T, N - a)
        if k == len(starts) - 1:
            la = N - a                                             # the last window runs to the read's end
        sel = np.nonzero((true_pos >= a) & (true_pos < a + la))[0]
        nz = rng.integers(-614, 615, nb) / 256.0 if per_chunk_noise else noise
        letters = truth[sel].copy()
        near_lo = (true_pos[sel] - a < 12) & (a > 0)
        near_hi = (a + la - true_pos[sel] <= 12) & (a + la < N)
        bad = near_lo | near_hi
        letters[bad] = np.frombuffer(b"N", np.uint8)[0]
        rows.append((a, la, 0, 0))
        calls.append((letters, (true_pos[sel] - a) + nz[sel]))
    S = max(len(c[0]) for c in calls)
    n = len(rows)
    bases = np.zeros((n, S), np.uint8)
    raw_pos = np.full((n, S), -1, np.float32)
    lengths = np.zeros(n, np.int32)
    for k, (letters, rp) in enumerate(calls):
        lengths[k] = len(letters)
        bases[k, :len(letters)] = letters
        raw_pos[k, :len(letters)] = rp.astype(np.float32)
    z = np.zeros((n, S), np.float32)
    return dict(truth=truth, windows=np.asarray(rows, np.int32), bases=bases, probs=np.full((n, S), 0.5, np.float32), lengths=lengths,
                raw_pos=raw_pos, raw_mass=np.where(raw_pos >= 0, 1, 0).astype(np.float32), event_pos=z - 1, event_mass=z)
