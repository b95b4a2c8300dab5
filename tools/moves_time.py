"""Timing: what the moves cost.  At the C3 shape -- 256 chunks, joint 300 + 30, beam 5, L = 48, device inputs and outputs -- one
synchronous rv_beam_search_all_dev beside one rv_beam_search_moves_dev into preallocated buffers, alternating round by round inside
one process: three rounds of `--reps` calls each per entry point.  A round's figure is the median of its calls; one JSON line gives,
for both entry points, the median of the three rounds and their spread (max - min), in ms per slab."""
import argparse, ctypes, gc, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ravvent_basecaller_amd as rv

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=256)
ap.add_argument("--raw", type=int, default=300)
ap.add_argument("--events", type=int, default=30)
ap.add_argument("--beam", type=int, default=5)
ap.add_argument("--L", type=int, default=48)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--persistent", type=int, default=1)
a = ap.parse_args()
B, T_r, T_e, W, L = a.chunks, a.raw, a.events, a.beam, a.L
raw, ev, _ = rv.synthetic.make_slab(B, T_r, T_e, seed=0)
d_raw, d_ev = torch.from_numpy(raw).cuda(), torch.from_numpy(ev).cuda()
bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=B, max_raw_len=T_r, max_event_len=T_e, max_output_len=L)
bc.init_random_weights(seed=22)
bc.set_option("persistent_decode", a.persistent)
beams = bc._beams_dev(B, L - 1, W)
moves = bc._moves_bufs(B, L - 1, W, True)
sb, sm = bc._beams_struct(beams), bc._moves_struct(moves)
S = ctypes.c_int32(0)
p = lambda t: ctypes.c_void_p(t.data_ptr())
torch.cuda.synchronize()


def call_all():
    bc._check(bc._lib.rv_beam_search_all_dev(bc._h, p(d_raw), p(d_ev), B, T_r, T_e, W, L, ctypes.byref(sb), ctypes.byref(S)), "rv_beam_search_all_dev")


def call_moves():
    bc._check(bc._lib.rv_beam_search_moves_dev(bc._h, p(d_raw), p(d_ev), B, T_r, T_e, W, L, ctypes.byref(sb), ctypes.byref(sm), ctypes.byref(S)),
              "rv_beam_search_moves_dev")


calls = {"all": call_all, "moves": call_moves}
gc.disable()
for fn in calls.values():
    for _ in range(5):
        fn()
rounds = {k: [] for k in calls}
for _ in range(a.rounds):                # alternating: both see the same machine
    for k, fn in calls.items():
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)       # synchronous calls: complete when they return
        rounds[k].append(float(np.median(ts)) * 1e3)
out = {"chunks": B, "T_r": T_r, "T_e": T_e, "beam": W, "L": L, "steps": S.value, "persistent_decode": a.persistent, "reps": a.reps}
for k, v in rounds.items():
    out[k + "_ms"] = {"median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4), "rounds": [round(x, 4) for x in v]}
out["moves_over_all"] = round(out["moves_ms"]["median"] / out["all_ms"]["median"], 4)
print(json.dumps(out))
bc.close()
