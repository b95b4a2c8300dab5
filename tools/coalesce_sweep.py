"""Diagnostic: the driver's stream (C3 slabs through the asynchronous calls, device inputs, reused outputs) by asynchronous depth and
slabs per group (option coalesce).  Per setting: `reps` timed regions of `steps` slabs each, every one started from an idle GPU and closed
by a device synchronisation like bench.py's, and one settled run of 4 x steps slabs.  Prints a markdown table row per setting.
Usage: coalesce_sweep.py [depth:n,n,...;depth:n,...] [steps] [reps]     e.g. "10:1,2,3,4,5;6:1,2;4:1,2" 20 5"""
import gc, os, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ravvent_basecaller_amd as rv
plan = sys.argv[1] if len(sys.argv) > 1 else "10:1,2,3,4,5;6:1,2;4:1,2"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
B, T_r, T_e, W, L = 256, 300, 30, 5, 48
warnings.simplefilter("ignore")
bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=B, max_raw_len=T_r, max_event_len=T_e, max_output_len=L)
bc.init_random_weights(seed=22)
bc.reuse_output_buffers = True
raw, ev, _ = rv.synthetic.make_slab(B, T_r, T_e, seed=0)
x = (torch.from_numpy(raw).cuda(), torch.from_numpy(ev).cuda())
want = [a.cpu().numpy().copy() for a in bc.beam_search_prediction(x, W, L)]
print(f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}; {steps} slabs per timed region, {reps} regions; ms per slab")
print("| depth | coalesce | median | min | max | settled | equal |")
print("|---|---|---|---|---|---|---|")
gc.disable()
for part in plan.split(";"):
    depth, ns = part.split(":")
    for n in (int(v) for v in ns.split(",")):
        bc.set_async_depth(int(depth)); bc.set_coalesce(n)
        outs = list(bc.beam_search_stream((x for _ in range(2 * int(depth) + 2)), W, L))      # warm-up: every context exists
        ok = all(np.array_equal(o[0].cpu().numpy(), want[0]) and np.array_equal(o[1].cpu().numpy(), want[1]) for o in outs[-2:])
        ms = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _o in bc.beam_search_stream((x for _ in range(steps)), W, L):
                pass
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / steps * 1e3)
        t0 = time.perf_counter()
        for _o in bc.beam_search_stream((x for _ in range(4 * steps)), W, L):
            pass
        torch.cuda.synchronize()
        settled = (time.perf_counter() - t0) / (4 * steps) * 1e3
        print(f"| {depth} | {n} | {sorted(ms)[len(ms) // 2]:.4f} | {min(ms):.4f} | {max(ms):.4f} | {settled:.4f} | {ok} |", flush=True)
bc.close()
