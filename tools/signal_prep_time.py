"""Wall clock of Basecaller.basecall_many with preparation on the host (device_prep=False: the C++ event detector, numpy scaling and the
chunk-range loop, read by read) against on the device (device_prep=True: rv_read_put_signals, one upload of the int16 samples and the
kernels of csrc/signal_prep.hip for the whole batch), in one process, the two settings in turns:

    one read       synthetic.make_read(9000, 11): the single-read latency, where one wave runs the peak pass alone
    16 reads       make_read(9000, 11 .. 26) in one call

Shape: bench.py's streamed line (joint 300 + 30, beam 5, L 48, 256 chunks per slab, 10 slabs in flight).  Per case 2 warm-up calls,
one discarded round, then REPEATS rounds; reported: every repeat, median and min - max, in ms and k chunks/s.  Then the preparation
alone (prepare_windows + put_read against put_signals), and the per-stage device times of rv_read_put_signals (profile scopes sp_*)."""
import gc, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ravvent_basecaller_amd as rv

B, T_r, T_e, W, L, DEPTH, REPEATS = 256, 300, 30, 5, 48, 10, 7
dl = rv.data_loader
bc = rv.Basecaller(128, 128, 128, dl.nuc_tk, "joint", dl.INPUT_PADDING, encoder_depth=2, decoder_depth=1, attention_type="luong",
                   beam_width=W, max_batch=B, max_raw_len=T_r, max_event_len=T_e, max_output_len=L)
bc.init_random_weights(seed=22)
bc.set_async_depth(DEPTH)

reads = [rv.synthetic.make_read(n_bases=9000, seed=11 + i)[0] for i in range(16)]
CASES = {"one read": reads[:1], "16 reads": reads}


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def line(name, ms, chunks=None):
    ms = np.asarray(ms)
    rate = "" if chunks is None else f"  {chunks / np.median(ms):8.1f} k chunks/s at the median"
    print(f"  {name:22s} {' '.join(f'{x:8.2f}' for x in ms)}   median {np.median(ms):8.2f} ms  ({ms.min():.2f} - {ms.max():.2f}){rate}", flush=True)


def prep_host(sigs):
    hs = []
    for s in sigs:
        rw = dl.prepare_windows(s, stride=6, max_raw_len=200, max_event_len=30)
        hs.append(bc.put_read(rw.raw_sc, rw.events_sc))
    return hs


def prep_device(sigs):
    return bc.put_signals(sigs, stride=6, max_raw_len=200, max_event_len=30)


gc.collect(); gc.disable()
for name, sigs in CASES.items():
    res = {}
    for dev in (False, True):
        for _ in range(2):
            res[dev] = bc.basecall_many(sigs, chunk_size=B, device_prep=dev)
    same = all(a.seq == b.seq and a.chunks_num == b.chunks_num for a, b in zip(res[False], res[True]))
    chunks = sum(r.chunks_num for r in res[True])
    print(f"{name}: {sum(len(s) for s in sigs)} samples, {chunks} chunks; device_prep calls the host path's bases: {same}", flush=True)
    t = {False: [], True: []}
    for rep in range(REPEATS + 1):
        for dev in (False, True):
            ms, _ = clock(lambda: bc.basecall_many(sigs, chunk_size=B, device_prep=dev))
            if rep:
                t[dev].append(ms)
    line("basecall_many host", t[False], chunks)
    line("basecall_many device", t[True], chunks)
    p = {False: [], True: []}
    for rep in range(REPEATS + 1):
        for dev in (False, True):
            ms, hs = clock(lambda: (prep_device if dev else prep_host)(sigs))
            for h in hs:
                h.drop()
            if rep:
                p[dev].append(ms)
    line("preparation host", p[False])
    line("preparation device", p[True])
    bc.set_option("profile", 1)
    bc.reset_profile()
    for _ in range(5):
        for h in prep_device(sigs):
            h.drop()
    prof = bc.profile()
    bc.set_option("profile", 0)
    stages = {k: v for k, v in prof.items() if k.startswith("sp_")}
    print("  device stages, ms per call: " + "  ".join(f"{k[3:]} {ms / n:.3f}" for k, (ms, n) in stages.items()) +
          f"  (sum {sum(ms / n for ms, n in stages.values()):.3f})", flush=True)
bc.close()
