"""Streamed chunks/s of window slabs against padded chunk tensors, at the C3 shape of bench.py's streamed line (joint 300 + 30, beam 5,
L 48, 256 chunks per slab, 10 slabs in flight), the windows cut from one long synthetic read.  Three paths in one process:

    windows      Basecaller.submit_windows(calls=True): the read uploaded once, a 24-byte table row per chunk
    padded host  Basecaller.submit_calls on host arrays: what a caller holding a read on the host had before
    padded dev   Basecaller.submit_beam_search on device tensors (bench.py's path: inputs and outputs stay on the device)

Each path: 5 warm-up steps, then 5 repeats of 20 steps (a step = one slab); reported per path: chunks/s of every repeat, their median
and min-max spread, the host time per submit, and the H2D bytes per chunk.  A fourth line, "windows expand", is the window path with
the padded tensors written by k_expand_windows in front of the unchanged kernels (group_inplace 0) instead of gathered in the lane."""
import gc, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ravvent_basecaller_amd as rv

B, T_r, T_e, W, L, DEPTH, STEPS, REPEATS, WARM = 256, 300, 30, 5, 48, 10, 20, 5, 5
dl = rv.data_loader
bc = rv.Basecaller(128, 128, 128, dl.nuc_tk, "joint", dl.INPUT_PADDING, encoder_depth=2, decoder_depth=1, attention_type="luong",
                   beam_width=W, max_batch=B, max_raw_len=T_r, max_event_len=T_e, max_output_len=L)
bc.init_random_weights(seed=22)
bc.set_async_depth(DEPTH)

sig, _ = rv.synthetic.make_read(n_bases=9000, seed=11)
rw = dl.prepare_windows(sig, stride=6, max_raw_len=T_r, max_event_len=T_e)
n_slabs = 4
assert len(rw) >= n_slabs * B, len(rw)
handle = bc.put_read(rw.raw_sc, rw.events_sc)
tables = [handle.table(rw.windows[i * B:(i + 1) * B]) for i in range(n_slabs)]
padded = [dl.expand_windows(rw.raw_sc, rw.events_sc, rw.windows[i * B:(i + 1) * B], T_r, T_e, dl.INPUT_PADDING) for i in range(n_slabs)]
device = [(torch.from_numpy(r).cuda(), torch.from_numpy(e).cuda()) for r, e in padded]
read_bytes = rw.raw_sc.nbytes + rw.events_sc.nbytes

# the three paths decode the same chunks: identical calls
want = [bc.beam_search_call_arrays(x, W, L) for x in padded]
got = [bc.beam_search_windows_call_arrays(t, W, L, T_r=T_r, T_e=T_e) for t in tables]
same = all(a.tobytes() == b.tobytes() for w_, g_ in zip(want, got) for a, b in zip(w_, g_))
print(f"read: {sig.size} samples, {rw.events_sc.shape[0]} events, {len(rw)} chunks; window calls == padded calls: {same}", flush=True)

PATHS = {
    "windows": (lambda i: bc.submit_windows(tables[i % n_slabs], W, L, calls=True, T_r=T_r, T_e=T_e), bc.collect_calls,
                24 + read_bytes / len(rw)),
    "padded host": (lambda i: bc.submit_calls(padded[i % n_slabs], W, L), bc.collect_calls, 4.0 * (T_r + 5 * T_e)),
    "padded dev": (lambda i: bc.submit_beam_search(device[i % n_slabs], W, L), bc.collect, 0.0),
}


def stream(submit, collect, steps):
    """`steps` slabs, DEPTH in flight -> (wall seconds, host seconds inside submit)."""
    queue, t_sub = [], 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        if len(queue) >= DEPTH:
            collect(queue.pop(0))
        a = time.perf_counter()
        queue.append(submit(i))
        t_sub += time.perf_counter() - a
    while queue:
        collect(queue.pop(0))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, t_sub


gc.collect(); gc.disable()
print(f"B={B} T=({T_r},{T_e}) W={W} L={L} depth={DEPTH}: {REPEATS} repeats of {STEPS} steps after {WARM} warm-up steps and one discarded round, the paths in turns; "
      f"coalesce in force: {int(bc.get_tensor('coalesce_stats')[3])}", flush=True)
# "windows expand": the same window slabs behind k_expand_windows instead of the in-lane gather (a group with group_inplace 0 takes it)
ORDER = ["windows", "windows expand", "padded host", "padded dev"]
PATHS["windows expand"] = PATHS["windows"]


def run(name, steps):
    submit, collect, _ = PATHS[name]
    if name == "windows expand":
        bc.set_option("group_inplace", 0)
    try:
        return stream(submit, collect, steps)
    finally:
        if name == "windows expand":
            bc.set_option("group_inplace", 1)


for name in ORDER:
    run(name, WARM)
# one discarded round: five warm-up steps never put DEPTH slabs in flight, and the first round that does pays for it once, whichever
# path goes first (its first repeat: 73 and 197 k chunks/s in two runs without this round, 340-350 k from the second repeat on)
for name in ORDER:
    run(name, STEPS)
rates, subs = {n: [] for n in ORDER}, {n: [] for n in ORDER}
for _ in range(REPEATS):
    for name in ORDER:
        dt, ts = run(name, STEPS)
        rates[name].append(B * STEPS / dt / 1e3); subs[name].append(ts / STEPS * 1e6)
for name in ORDER:
    r = rates[name]
    print(f"  {name:14s}: " + " ".join(f"{v:6.1f}" for v in r) + f" k chunks/s; median {np.median(r):6.1f}, spread {min(r):.1f}-{max(r):.1f}"
          f"; submit {np.median(subs[name]):5.1f} us; H2D {PATHS[name][2]:7.1f} B/chunk", flush=True)
print(f"read_stats (allocations, alive, puts, slots, expand launches): {bc.get_tensor('read_stats').astype(int).tolist()}")
handle.drop()
bc.close()
