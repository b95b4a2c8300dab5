"""What positions cost (profiles/signal_map.md): `basecall_many(..., moves=True)` against `moves=False`, and `align` against
`teacher_forced_prediction`, on this build.

    python tools/signal_map_time.py [--reads 8] [--bases 6000] [--repeats 5]

basecall_many: wall time over a batch of synthetic reads, the two settings in turns, one discarded run then `repeats` timed ones, at
the handle's default depth (2 slabs in flight, nothing coalesced) and at depth 10 with `coalesce` -1 (groups of five for moves=False;
a positions slab is never coalesced) and 0 (no groups for either: what is left is the cost of the records and the finalize).
align: per-launch time on one slab of 256 chunks, joint 300 + 30, L = 48, device tensors, 20 calls per round, in turns.
Prints one line per figure: median and range."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _emitting(rv, cfg):
    flat = rv.weights.init_weights(cfg, seed=22, gain=3.0)
    letters = [t for t in range(cfg.vocab) if t not in (cfg.start_token, cfg.end_token, cfg.pad_token)]
    flat["b_fc"][letters] += 1.5
    flat["b_fc"][cfg.end_token] -= 1.0
    return flat


def _turns(fns, repeats):
    """fns: name -> callable; each runs once unmeasured, then `repeats` times in turns -> name -> list of seconds."""
    out = {k: [] for k in fns}
    for k, f in fns.items():
        f()
    for _ in range(repeats):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            out[k].append(time.perf_counter() - t0)
    return out


def _fmt(xs, scale=1e3, unit="ms"):
    xs = np.asarray(xs) * scale
    return f"median {np.median(xs):.3f} {unit}, range {xs.min():.3f} - {xs.max():.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8)
    ap.add_argument("--bases", type=int, default=6000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import ravvent_basecaller_amd as rv

    sigs = [np.asarray(rv.synthetic.make_read(n_bases=a.bases, seed=s)[0]).astype(np.int16) for s in range(a.reads)]
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=1024, max_raw_len=200, max_event_len=30, max_output_len=32)
    bc.set_weights_flat(_emitting(rv, bc.cfg))
    n_chunks = sum(r.chunks_num for r in bc.basecall_many(sigs, max_output_len=32, chunk_size=256))
    print(f"{a.reads} reads of {a.bases} bases, {sum(len(s) for s in sigs)} samples, {n_chunks} chunks, slabs of 256, L = 32, beam 5")
    for depth, co in ((2, -1), (10, -1), (10, 0)):
        bc.set_async_depth(depth)
        bc.set_coalesce(co)
        for prep in (False, True):
            t = _turns({m: (lambda m=m: bc.basecall_many(sigs, max_output_len=32, chunk_size=256, device_prep=prep, moves=m)) for m in (False, True)},
                       a.repeats)
            ratio = np.median(t[True]) / np.median(t[False])
            print(f"basecall_many depth {depth} coalesce {co} device_prep {int(prep)}: moves=False {_fmt(t[False])}; moves=True {_fmt(t[True])}; "
                  f"ratio of medians {ratio:.3f}")
    bc.close()

    B, TR, TE, L = 256, 300, 30, 48
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=B, max_raw_len=TR, max_event_len=TE, max_output_len=L)
    bc.set_weights_flat(_emitting(rv, bc.cfg))
    raw, ev, _ = rv.synthetic.make_slab(B, TR, TE, seed=1)
    x = (torch.from_numpy(raw).cuda(), torch.from_numpy(ev).cuda())
    tg = torch.from_numpy(np.random.default_rng(1).integers(3, 7, (B, L)).astype(np.int32)).cuda()
    for name, opts in (("persistent", dict(persistent_decode=1)), ("per-step", dict(persistent_decode=0))):
        for k, v in opts.items():
            bc.set_option(k, v)

        def rounds(f):
            def run():
                for _ in range(20):
                    f()
                torch.cuda.synchronize()
            return run
        t = _turns({"teacher_forced_prediction": rounds(lambda: bc.teacher_forced_prediction(x, tg)), "align": rounds(lambda: bc.align(x, tg))},
                   a.repeats)
        per = {k: np.asarray(v) / 20 for k, v in t.items()}
        print(f"{name} decode, 256 chunks 300 + 30, L = 48: teacher_forced_prediction {_fmt(per['teacher_forced_prediction'])}; "
              f"align {_fmt(per['align'])}; ratio of medians {np.median(per['align']) / np.median(per['teacher_forced_prediction']):.3f}")
    bc.close()


if __name__ == "__main__":
    main()
