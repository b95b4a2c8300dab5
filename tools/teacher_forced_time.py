"""Timing: one synchronous forced call (Basecaller._teacher_forced: rv_teacher_forced_dev, decode + scoring) beside one greedy call at the
bench's shape -- 256 chunks, joint 300 + 30, L = 48, device inputs -- on base-emitting weights with the end token pushed down, so that the
greedy search runs all 47 steps like the forced decode.  The two calls alternate inside one process; medians and the spread are printed
as one JSON line.  A build without the forced call (an earlier commit on PYTHONPATH) times the greedy call alone."""
import argparse, gc, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ravvent_basecaller_amd as rv

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=256)
ap.add_argument("--raw", type=int, default=300)
ap.add_argument("--events", type=int, default=30)
ap.add_argument("--L", type=int, default=48)
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--persistent", type=int, default=1)
a = ap.parse_args()
B, T_r, T_e, L = a.chunks, a.raw, a.events, a.L
raw, ev, _ = rv.synthetic.make_slab(B, T_r, T_e, seed=0)
x = (torch.from_numpy(raw).cuda(), torch.from_numpy(ev).cuda())
bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=B, max_raw_len=T_r, max_event_len=T_e, max_output_len=L)
flat = rv.weights.init_weights(bc.cfg, seed=22, gain=3.0)
flat["b_fc"][3:7] += 1.5
flat["b_fc"][bc.cfg.end_token] -= 30.0          # no chunk ever emits the end token: the greedy loop runs L - 1 steps
bc.set_weights_flat(flat)
bc.set_option("persistent_decode", a.persistent)
tok, _ = bc.greedy_search_prediction(x, L)
S = tok.shape[1]
assert S == L - 1, f"the greedy search stopped after {S} steps"
calls = {"greedy": lambda: bc.greedy_search_prediction(x, L)}
if hasattr(bc, "_teacher_forced"):
    target = torch.cat([torch.full((B, 1), int(bc.cfg.start_token), dtype=torch.int32), tok.cpu()], dim=1).cuda()
    calls["forced"] = lambda: bc._teacher_forced(x, target, (0, 1, 2))
gc.disable()
for fn in calls.values():
    for _ in range(8):
        fn()
ts = {k: [] for k in calls}
for _ in range(a.reps):              # alternating: both see the same machine
    for k, fn in calls.items():
        t = time.perf_counter(); fn(); ts[k].append(time.perf_counter() - t)       # synchronous calls: complete when they return
out = {"chunks": B, "T_r": T_r, "T_e": T_e, "L": L, "steps": S, "persistent_decode": a.persistent, "reps": a.reps}
for k, v in ts.items():
    v = np.asarray(v) * 1e3
    out[k + "_ms"] = {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4),
                      "per_step_us": round(float(np.median(v)) / S * 1e3, 2)}
print(json.dumps(out))
