"""What the two merges cost (profiles/stitch.md): `basecall_many(..., merge="position")` against `moves=True` and `moves=False` (both
with the alignment merge), on this build.  After tools/signal_map_time.py: the same 8 synthetic reads, slabs of 256 chunks, L = 32.

    python tools/stitch_time.py [--reads 8] [--bases 6000] [--repeats 5]

Wall time of one basecall_many over the batch, the three forms in turns in one session, one discarded run each and then `repeats`
timed ones, with host and with device preparation, at the handle's default depth (2 slabs in flight).  Prints one line per
preparation (median and range of each form, and whether "position" is slower than moves=True by more than half of moves=True's own
max - min spread), then the per-scope device times of one profiled merge="position" call (option "profile" 1)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.signal_map_time import _emitting, _fmt, _turns      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8)
    ap.add_argument("--bases", type=int, default=6000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import ravvent_basecaller_amd as rv

    sigs = [np.asarray(rv.synthetic.make_read(n_bases=a.bases, seed=s)[0]).astype(np.int16) for s in range(a.reads)]
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=1024, max_raw_len=200, max_event_len=30, max_output_len=32)
    bc.set_weights_flat(_emitting(rv, bc.cfg))
    kw = dict(max_output_len=32, chunk_size=256)
    plain = bc.basecall_many(sigs, **kw)
    stitched = bc.basecall_many(sigs, merge="position", **kw)
    print(f"{a.reads} reads of {a.bases} bases, {sum(len(s) for s in sigs)} samples, {sum(r.chunks_num for r in plain)} chunks, slabs of 256, "
          f"L = 32, beam 5; bases per batch: align {sum(len(r.seq) for r in plain)}, position {sum(len(r.seq) for r in stitched)}")
    forms = {"position": dict(merge="position"), "moves=True": dict(moves=True), "moves=False": dict()}
    for prep in (False, True):
        t = _turns({k: (lambda v=v: bc.basecall_many(sigs, device_prep=prep, **kw, **v)) for k, v in forms.items()}, a.repeats)
        spread = max(t["moves=True"]) - min(t["moves=True"])
        slower = np.median(t["position"]) - np.median(t["moves=True"]) > 0.5 * spread
        print(f"basecall_many device_prep {int(prep)}: " + "; ".join(f"{k} {_fmt(v)}" for k, v in t.items()) +
              f"; position / moves=True {np.median(t['position']) / np.median(t['moves=True']):.3f}, position / moves=False "
              f"{np.median(t['position']) / np.median(t['moves=False']):.3f}; position slower than moves=True by more than half its spread: {slower}")
    for prep in (False, True):
        bc.set_option("profile", 1)
        bc.reset_profile()
        t0 = time.perf_counter()
        bc.basecall_many(sigs, device_prep=prep, merge="position", **kw)
        wall = time.perf_counter() - t0
        prof = bc.profile()
        bc.set_option("profile", 0)
        top = sorted(prof.items(), key=lambda kv: -kv[1][0])
        print(f"profiled merge='position' call, device_prep {int(prep)}: wall {wall * 1e3:.1f} ms; device ms by scope: " +
              ", ".join(f"{k} {ms:.3f} ({n})" for k, (ms, n) in top if ms >= 0.01 or k.startswith("stitch_")))
    bc.close()


if __name__ == "__main__":
    main()
