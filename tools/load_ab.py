"""Two builds of libravvent_hip.so, held to each other byte for byte on what rv_load_weights leaves on the device -- seen through
everything a decode computes from it -- and timed on the load itself.

    python tools/load_ab.py BASE.so NEW.so [--out DIR]

For each library one fresh child process (the library chosen through RAVVENT_HIP_LIB, under its own time limit; the second starts only
if the first exited 0) loads weights and runs a fixed set of small cases: 17 chunks (one full sixteen-chunk group and a remainder) of
96 samples + 24 events, 12 output positions, beam 5 and greedy, persist_taps on:

    bilstm enc 2 / dec 1 Luong, the same under weight_parts 1, Bahdanau, enc 3 / dec 2, dec 3, bigru enc 2 / dec 1, bigru enc 1 / dec 2

and saves tokens, scores, greedy tokens and logits, enc_output, and step_logits / projected_memory where the call leaves them.  The
parent compares the two saves array by array on their bytes, and prints the wall time of Basecaller.set_weights_flat (median and min-max
of LOADS loads, enc 2 / dec 1 and enc 3 / dec 2) of both.  Exit status 1 if anything differs."""
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

B, T_R, T_E, W, L, LOADS = 17, 96, 24, 5, 12, 9
# name: (rnn, encoder depth, decoder depth, attention, weight_parts)
CASES = {
    "bilstm-2-1": ("bilstm", 2, 1, "luong", 2),
    "bilstm-2-1-parts1": ("bilstm", 2, 1, "luong", 1),
    "bilstm-2-1-bahdanau": ("bilstm", 2, 1, "bahdanau", 2),
    "bilstm-3-2": ("bilstm", 3, 2, "luong", 2),
    "bilstm-2-3": ("bilstm", 2, 3, "luong", 2),
    "bigru-2-1": ("bigru", 2, 1, "luong", 2),
    "bigru-1-2": ("bigru", 1, 2, "luong", 2),
}
TIMED = ("bilstm-2-1", "bilstm-3-2")


def child(out):
    import torch
    import ravvent_basecaller_amd as rv
    dl = rv.data_loader
    raw, ev, _ = rv.synthetic.make_slab(B, T_R, T_E, seed=3)
    x = (torch.from_numpy(raw).cuda(), torch.from_numpy(ev).cuda())
    save = {}
    for i, (name, (rnn, enc, dec, att, parts)) in enumerate(CASES.items()):
        bc = rv.Basecaller(128, 128, 128, dl.nuc_tk, "joint", dl.INPUT_PADDING, encoder_depth=enc, decoder_depth=dec, rnn_type=rnn,
                           attention_type=att, honor_attention_type=True, beam_width=W, max_batch=32, max_raw_len=T_R, max_event_len=T_E,
                           max_output_len=L)
        if parts != 2:
            bc.set_weight_parts(parts)
        flat = rv.weights.init_weights(bc.cfg, seed=40 + i, scheme="hash")
        flat["b_fc"][3:7] += 1.5                  # favour a/c/g/t and keep the end token rare: every step of every chunk decodes
        flat["b_fc"][bc.cfg.end_token] -= 3.0
        bc.set_weights_flat(flat)
        if name in TIMED:
            t = []
            for _ in range(LOADS):
                t0 = time.perf_counter()
                bc.set_weights_flat(flat)
                t.append((time.perf_counter() - t0) * 1e3)
            save[name + "/load_ms"] = np.array(t)
        bc.set_option("persist_taps", 1)

        def taps(prefix, names):
            for n in names:
                try:
                    save[f"{name}/{prefix}_{n}"] = bc.get_tensor(n)
                except Exception:                 # this call leaves no such tensor (no persistent decode for the configuration)
                    pass
        tok, sc = bc.beam_search_prediction(x, W, L)
        save[name + "/beam_tokens"], save[name + "/beam_scores"] = tok.cpu().numpy(), sc.cpu().numpy()
        taps("beam", ["enc_output", "projected_memory"])
        if name + "/beam_projected_memory" in save:                    # (the persistent decode ran: its taps are this call's)
            taps("beam", ["step_logits"])
        tok, lg = bc.greedy_search_prediction(x, L)
        save[name + "/greedy_tokens"], save[name + "/greedy_logits"] = tok.cpu().numpy(), lg.cpu().numpy()
        taps("greedy", ["step_logits"])
        bc.close()
    np.savez(out, **save)


def main():
    base, new = sys.argv[1], sys.argv[2]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "."
    os.makedirs(out, exist_ok=True)
    saves = []
    for tag, lib in (("base", base), ("new", new)):
        path = os.path.join(out, f"load_ab_{tag}.npz")
        rc = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", path],
                            env=dict(os.environ, RAVVENT_HIP_LIB=os.path.abspath(lib))).returncode
        if rc != 0:
            sys.exit(f"{tag} ({lib}): the child exited {rc}; nothing more is started")
        saves.append(np.load(path))
    a, b = saves
    bad = 0
    print(f"base = {base}, new = {new}; {B} chunks of {T_R} + {T_E}, beam {W}, L {L}\n")
    print("| case | arrays compared | bytes | differing arrays |")
    print("|---|---|---|---|")
    for name in CASES:
        keys = sorted(k for k in set(a.files) | set(b.files) if k.startswith(name + "/") and not k.endswith("load_ms"))
        diff = [k.split("/", 1)[1] for k in keys if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
        bad += len(diff)
        print(f"| {name} | {', '.join(k.split('/', 1)[1] for k in keys)} | {sum(a[k].nbytes for k in keys if k in a.files)} | {', '.join(diff) or 'none'} |")
    print("\n| set_weights_flat, ms | base: median (min-max) | new: median (min-max) | new / base |")
    print("|---|---|---|---|")
    for name in TIMED:
        ta, tb = a[name + "/load_ms"], b[name + "/load_ms"]
        print(f"| {name} | {np.median(ta):.1f} ({ta.min():.1f}-{ta.max():.1f}) | {np.median(tb):.1f} ({tb.min():.1f}-{tb.max():.1f}) | {np.median(tb) / np.median(ta):.3f} |")
    print("\n" + ("every array equal byte for byte" if not bad else f"{bad} arrays DIFFER"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
