"""rnn_type 'bigru' beside 'bilstm' at the C3 shape (joint 300 + 30, beam 5, 256 chunks per slab, L 48, Keras weights of seed 22), both
on the per-step decode (the BiLSTM handle with persistent_decode 0; the GRU handle at its default), and both on the one-launch
persistent decode (a second GRU handle under gru_persistent 1, a second BiLSTM handle at its default), one process, the four handles
in turns within every repeat.

Per repeat and handle: STEPS synchronous calls under profile 2 (events around every launch, the decode's kernels launched one by one)
for the scopes, then STEPS synchronous calls under profile 0 for the whole slab's chunks/s.  One discarded round first.  Printed, as the
tables of profiles/gru.md: per-launch time of gru_rec_* beside lstm_rec_* of the same layer, of dec_cell_gru beside dec_cell, of the
input-projection GEMMs (three column blocks beside four), the whole-slab rate of both, each with its median and its min-max spread over
the repeats, and the GRU / LSTM ratio of the medians beside the LSTM scope's own relative spread; then (a) dec_persist_gru per launch
beside the BiLSTM handle's dec_persist and (b) the GRU handle's whole-slab rate with gru_persistent on and off, the gain beside the
(max - min) / 2 spread of the rate with the option off.

    python tools/gru_time.py"""
import gc, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ravvent_basecaller_amd as rv

B, T_r, T_e, W, L, STEPS, REPEATS = 256, 300, 30, 5, 48, 10, 5
dl = rv.data_loader


def handle(rnn, persistent=False):
    bc = rv.Basecaller(128, 128, 128, dl.nuc_tk, "joint", dl.INPUT_PADDING, encoder_depth=2, decoder_depth=1, rnn_type=rnn,
                       attention_type="luong", beam_width=W, max_batch=B, max_raw_len=T_r, max_event_len=T_e, max_output_len=L)
    bc.init_random_weights(seed=22)
    if not persistent:
        bc.set_option("persistent_decode", 0)
    elif rnn == "bigru":
        bc.set_gru_persistent(True)
    return bc


handles = {"bigru": handle("bigru"), "bilstm": handle("bilstm"), "bigru-persistent": handle("bigru", True), "bilstm-persistent": handle("bilstm", True)}
slabs = [rv.synthetic.make_slab(B, T_r, T_e, seed=s)[:2] for s in range(4)]
device = [(torch.from_numpy(r).cuda(), torch.from_numpy(e).cuda()) for r, e in slabs]
PAIRS = [("gru_rec_raw_l0", "lstm_rec_raw_l0"), ("gru_rec_event_l0", "lstm_rec_event_l0"), ("gru_rec_raw_l1p", "lstm_rec_raw_l1p"),
         ("gru_rec_event_l1p", "lstm_rec_event_l1p"), ("gemm_inproj_raw", "gemm_inproj_raw"), ("gemm_inproj_event", "gemm_inproj_event"),
         ("dec_cell_gru", "dec_cell"), ("dec_attend", "dec_attend")]


def scopes(bc):
    bc.set_option("profile", 2)
    bc.reset_profile()
    for i in range(STEPS):
        bc.beam_search_prediction(device[i % 4], W, L)
    prof = bc.profile()
    bc.set_option("profile", 0)
    return {k: ms / n for k, (ms, n) in prof.items() if n}


def rate(bc):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(STEPS):
        bc.beam_search_prediction(device[i % 4], W, L)
    torch.cuda.synchronize()
    return B * STEPS / (time.perf_counter() - t0) / 1e3


gc.collect(); gc.disable()
per = {n: [] for n in handles}
rates = {n: [] for n in handles}
for rep in range(REPEATS + 1):
    for name, bc in handles.items():
        s, r = scopes(bc), rate(bc)
        if rep:                                  # (the first round is discarded)
            per[name].append(s); rates[name].append(r)


def stat(v):
    return float(np.median(v)), float(min(v)), float(max(v))


print(f"B={B} T=({T_r},{T_e}) W={W} L={L}, per-step decode on both handles; {REPEATS} repeats of {STEPS} synchronous calls, the handles in turns, one round discarded\n")
print("| scope (bigru / bilstm) | bigru ms per launch: median (min-max) | bilstm ms per launch: median (min-max) | ratio of medians | bilstm's own spread |")
print("|---|---|---|---|---|")
for g, l in PAIRS:
    gv, lv = [p[g] for p in per["bigru"] if g in p], [p[l] for p in per["bilstm"] if l in p]
    if not gv or not lv:
        print(f"| {g} / {l} | {'-' if not gv else ''} | {'-' if not lv else ''} | - | - |")
        continue
    (gm, g0, g1), (lm, l0, l1) = stat(gv), stat(lv)
    print(f"| {g} / {l} | {gm:.4f} ({g0:.4f}-{g1:.4f}) | {lm:.4f} ({l0:.4f}-{l1:.4f}) | {gm / lm:.3f} | +-{100 * (l1 - l0) / (2 * lm):.1f} % |")
(gm, g0, g1), (lm, l0, l1) = stat(rates["bigru"]), stat(rates["bilstm"])
print(f"\nwhole slab, synchronous calls: bigru {gm:.1f} k chunks/s ({g0:.1f}-{g1:.1f}), bilstm on the per-step decode {lm:.1f} ({l0:.1f}-{l1:.1f}); ratio {gm / lm:.3f}")
print("per repeat, k chunks/s: bigru " + " ".join(f"{v:.1f}" for v in rates["bigru"]) + "; bilstm " + " ".join(f"{v:.1f}" for v in rates["bilstm"]))

# (a) the persistent decode's one launch, GRU beside LSTM
gv, lv = [p["dec_persist_gru"] for p in per["bigru-persistent"]], [p["dec_persist"] for p in per["bilstm-persistent"]]
(gm, g0, g1), (lm, l0, l1) = stat(gv), stat(lv)
print(f"\n(a) per launch, ms: dec_persist_gru {gm:.4f} ({g0:.4f}-{g1:.4f}), dec_persist {lm:.4f} ({l0:.4f}-{l1:.4f}); ratio of medians {gm / lm:.3f}, "
      f"dec_persist's own spread +-{100 * (l1 - l0) / (2 * lm):.1f} %")
# (b) the GRU handle's whole slab, option on and off
(pm, p0, p1), (om, o0, o1) = stat(rates["bigru-persistent"]), stat(rates["bigru"])
print(f"(b) whole slab, synchronous calls, k chunks/s: bigru with gru_persistent 1 {pm:.1f} ({p0:.1f}-{p1:.1f}), with 0 {om:.1f} ({o0:.1f}-{o1:.1f}); "
      f"gain {pm - om:.1f} against off's own (max - min) / 2 = {(o1 - o0) / 2:.1f}; the bilstm default {stat(rates['bilstm-persistent'])[0]:.1f}")
print("per repeat, k chunks/s: on " + " ".join(f"{v:.1f}" for v in rates["bigru-persistent"]) + "; off " + " ".join(f"{v:.1f}" for v in rates["bigru"]))
for bc in handles.values():
    bc.close()
