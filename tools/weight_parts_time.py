"""Option weight_parts at the C3 shape of bench.py's streamed line (joint 300 + 30, beam 5, L 48, 256 chunks per
slab, 10 slabs in flight, Keras weights of seed 22).  Three paths in one process, in turns within every repeat:

    parts 2        the default: every weight as two f16 parts, k_dec_persist
    parts 1 / 2p   weight_parts 1 with one_part_kernels 0: the rounded weights on the two-part kernels (second parts zero)
    parts 1 / 1p   weight_parts 1 with one_part_kernels 1: k_dec_persist_1p, one MFMA and half the stream per (k-step, gate) pair

Each path: 5 warm-up steps, one discarded round, then 5 repeats of 20 steps (a step = one slab).  Reported per path: streamed k chunks/s
of every repeat with median and min-max, and the decode launch alone (option profile 3: events around the decode launch only) from a
pass of synchronous calls.  Then, on the same slabs, what a user trades: the share of chunks whose beam-0 call differs between
weight_parts 2 and 1, and the largest difference of a per-base probability where the calls agree.

    python tools/weight_parts_time.py            # the timing and the accuracy figures
    python tools/weight_parts_time.py --stamps   # instead: the step stamps of workgroup 0 (RV_DBG_STAMPS), two-part beside one-part"""
import gc, os, sys, time
STAMPS = "--stamps" in sys.argv
if STAMPS:
    os.environ["RV_DBG_STAMPS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ravvent_basecaller_amd as rv

B, T_r, T_e, W, L, DEPTH, STEPS, REPEATS, WARM = 256, 300, 30, 5, 48, 10, 20, 5, 5
dl = rv.data_loader


# ONE handle serves the three paths: its weights are loaded again in the other mode between them (outside every timed region).  Two
# handles of one process do not stream alike -- ten streams each on four hardware queues; the one created second streamed 11 % faster
# on the same kernel -- so they cannot carry a comparison between modes
bc = rv.Basecaller(128, 128, 128, dl.nuc_tk, "joint", dl.INPUT_PADDING, encoder_depth=2, decoder_depth=1, attention_type="luong",
                   beam_width=W, max_batch=B, max_raw_len=T_r, max_event_len=T_e, max_output_len=L)
bc.init_random_weights(seed=22)
bc.set_async_depth(DEPTH)
n_slabs = 4
slabs = [rv.synthetic.make_slab(B, T_r, T_e, seed=s)[:2] for s in range(n_slabs)]
device = [(torch.from_numpy(r).cuda(), torch.from_numpy(e).cuda()) for r, e in slabs]
PATHS = {"parts 2": (2, 1), "parts 1 / 2p": (1, 0), "parts 1 / 1p": (1, 1)}
ORDER = list(PATHS)


def select(name):
    parts, one = PATHS[name]
    if bc.weight_parts_loaded != parts:
        bc.set_weight_parts(parts)
    bc.set_option("one_part_kernels", one)
    return bc


if STAMPS:
    pn = [("gates", 0, 2), ("att-h", 2, 3), ("scores", 3, 4), ("softmax", 4, 5), ("context", 5, 6), ("merge", 6, 8), ("logits", 8, 9),
          ("beam||cell product", 9, 10)]
    for name in ORDER:
        select(name)
        for _ in range(3):
            bc.beam_search_prediction(device[0], W, L)
            ts = bc.get_tensor("dbg_stamps")
            print(f"{name:13s}: " + " ".join(f"{n}={ts[j] - ts[i]:.0f}" for n, i, j in pn), "step total", ts[10] - ts[0],
                  f"| beam step (wave 0) {ts[11] - ts[9]:.0f}, wave 1's cell product {ts[13] - ts[12]:.0f} (starts {ts[12] - ts[9]:.0f} after the logits barrier)")
    sys.exit(0)


def stream(bc, steps):
    queue = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        if len(queue) >= DEPTH:
            bc.collect(queue.pop(0))
        queue.append(bc.submit_beam_search(device[i % n_slabs], W, L))
    while queue:
        bc.collect(queue.pop(0))
    torch.cuda.synchronize()
    return time.perf_counter() - t0


gc.collect(); gc.disable()
print(f"B={B} T=({T_r},{T_e}) W={W} L={L} depth={DEPTH}: {REPEATS} repeats of {STEPS} steps after {WARM} warm-up steps and one discarded round, the paths in turns", flush=True)
for name in ORDER:
    stream(select(name), WARM)
for name in ORDER:
    stream(select(name), STEPS)
rates = {n: [] for n in ORDER}
for _ in range(REPEATS):
    for name in ORDER:
        rates[name].append(B * STEPS / stream(select(name), STEPS) / 1e3)
for name in ORDER:
    r = rates[name]
    print(f"  {name:13s}: " + " ".join(f"{v:6.1f}" for v in r) + f" k chunks/s; median {np.median(r):6.1f}, spread {min(r):.1f}-{max(r):.1f}", flush=True)

# the decode launch alone: synchronous calls under profile 3, the paths in turns within every repeat
launch, forms = {n: [] for n in ORDER}, {}
bc.set_option("profile", 3)
for rep in range(REPEATS + 1):
    for name in ORDER:
        select(name)
        bc.reset_profile()
        for i in range(STEPS):
            bc.beam_search_prediction(device[i % n_slabs], W, L)
        ms, n = bc.profile()["dec_persist"]
        if rep:                                # (the first round is discarded)
            launch[name].append(ms / n)
        forms[name] = [tuple(int(v) for v in r) for r in bc.get_tensor("kernel_forms").reshape(-1, 5) if r[0] in (0, 8)]
bc.set_option("profile", 0)
for name in ORDER:
    v = launch[name]
    print(f"  {name:13s}: decode launch " + " ".join(f"{x:.4f}" for x in v) + f" ms; median {np.median(v):.4f}, spread {min(v):.4f}-{max(v):.4f}; form {forms[name]}", flush=True)

# what a user trades: beam-0 calls of weight_parts 2 against 1 on the same chunks
differ, total, dmax = 0, 0, 0.0
calls2 = [select("parts 2").beam_search_call_arrays(x, W, L) for x in slabs]
calls1 = [select("parts 1 / 1p").beam_search_call_arrays(x, W, L) for x in slabs]
for (b2, p2, l2), (b1, p1, l1) in zip(calls2, calls1):
    for c in range(B):
        same = l2[c] == l1[c] and (b2[c, :l2[c]] == b1[c, :l1[c]]).all()
        total += 1
        differ += 0 if same else 1
        if same and l2[c]:
            dmax = max(dmax, float(np.abs(p2[c, :l2[c]] - p1[c, :l1[c]]).max()))
print(f"accuracy: {differ} of {total} chunks ({100.0 * differ / total:.2f} %) call a different beam-0 sequence under weight_parts 1; "
      f"largest per-base probability difference where the calls agree {dmax:.2e}")
bc.close()
