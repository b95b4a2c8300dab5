"""Every listed instantiation of the decode and recurrence kernels, held to fp64.

Each kernel family keeps its instantiations in one list (decode.hip: for_each_persist_form, for_each_attend_form; lstm_rec.hip:
for_each_rec_form / _tw_form / _proj_form; lstm_mx.hip: for_each_mx_form, for_each_inproj_form), and the launchers pick from those
lists.  rv_get_tensor("kernel_forms") names the forms the last call launched, "kernel_form_list" every form the lists hold.  Every
call here is checked against the fp64 oracle -- within 1e-4, and no further from it than twice the oracle's numpy fp32 twin plus 5e-6
(test_parity_gpu._assert_twin) -- and for the form it was meant to run; each test then asserts that the forms its calls
ran are exactly its family's part of the list, so a form added to a list without a case here fails by name.  Forms no call can
reach are named in EXCLUDED with the rule that keeps them out.

The slabs carry the mask patterns where row-group and live-step logic goes wrong (_slab), memory lengths sit on the edges of each
kernel's bands (k_dec_persist<.., NIT, ..> serves T_m <= 32 NIT, k_dec_attend<W, TB> T_m <= 32 TB), and the weights (gain 1.5, an
end-token bias) make chunks finish at different steps."""
import numpy as np
import pytest

from test_bench_config_gpu import _agreeing_steps
from test_parity_gpu import (_assert_twin, _beam_errors, _check_alignments, _greedy_errors, _near_tie_gap, _twin_beam,
                             _twin_greedy)

pytestmark = pytest.mark.gpu

TOL = 1e-4          # against fp64
FORM_TOL = 2e-5     # between two forms on the same slab (the convention of test_matrix_attention_matches_fp32_rows_and_oracle)
B, V = 6, 7

# kernel ids of the "kernel_forms" rows (include/ravvent_hip.h)
PERSIST, FLASH, ATTEND, REC, REC_TW, REC_PROJ, REC_MX, INPROJ = range(8)
DECODE = (PERSIST, FLASH, ATTEND)
ENCODER = (REC, REC_TW, REC_PROJ, REC_MX, INPROJ)


def _f(*p):
    return tuple(p) + (0,) * (5 - len(p))


# listed forms that no call can launch, and the rule that keeps them out
EXCLUDED = {
    **{_f(FLASH, W, NT): "the single-pass attend needs Luong and an effective beam <= 5 (ravvent_hip.cpp, record_slab: lflash)"
       for W in (6, 7, 8) for NT in (256, 512)},
    _f(INPROJ, 1): "raw layer 0 always takes its one-feature projection in the lane (run_encoder), and wide_recurrence refuses a raw "
                   "window that does not fit",
}

# k_dec_persist families: name -> (attention, decoder cells, widest beam, {ATT: the options that select it (dec_persist_form)})
PERSIST_FAMILIES = {
    "luong1": ("luong", 1, 8, {0: dict(matrix_attention=0, matrix_cell=0), 2: dict(matrix_attention=1, matrix_cell=0),
                               3: dict(matrix_attention=1, matrix_cell=1)}),
    "bahdanau1": ("bahdanau", 1, 8, {1: dict(matrix_attention=1, matrix_cell=0), 4: dict(matrix_attention=1, matrix_cell=1)}),
    "luong2": ("luong", 2, 5, {0: dict(matrix_attention=1, matrix_cell=0), 3: dict(matrix_attention=1, matrix_cell=1)}),
}
PERSIST_BANDS = {2: (33, 64), 8: (65, 256), 11: (257, 352)}     # NIT -> the two edges of the T_m it serves
ATTEND_BANDS = {2: (64, 64), 7: (65, 224), 11: (225, 352)}       # TB -> the same for k_dec_attend


def _family(row):
    """The test that covers a listed form."""
    if row[0] == PERSIST:
        return next((f"persist:{fam}" for fam, (_, D, _, atts) in PERSIST_FAMILIES.items() if row[3] == D and row[4] in atts), None)
    return {FLASH: "flash", ATTEND: "attend", REC: "fma", REC_TW: "fma", REC_PROJ: "fma", REC_MX: "mx", INPROJ: "mx"}.get(row[0])


FAMILIES = [f"persist:{fam}" for fam in PERSIST_FAMILIES] + ["flash", "attend", "fma", "mx"]


def _rows(bc, name):
    return {tuple(int(v) for v in r) for r in bc.get_tensor(name).reshape(-1, 5)}


def _assert_family_ran(bc, fam, ran):
    """The forms a family's calls ran == its part of kernel_form_list, less the named exclusions."""
    listed = {r for r in _rows(bc, "kernel_form_list") if _family(r) == fam}
    ran = {r for r in ran if _family(r) == fam}
    excluded = listed & set(EXCLUDED)
    assert not ran & excluded, f"{fam}: excluded forms ran: {sorted(ran & excluded)}"
    missing = listed - excluded - ran
    assert not missing, f"{fam}: listed forms that no case runs: {sorted(missing)}"
    assert ran <= listed, f"{fam}: forms ran that the lists do not hold: {sorted(ran - listed)}"
    print(f"{fam}: {len(ran)}/{len(listed)} listed forms ran" +
          "".join(f"; excluded {r}: {EXCLUDED[r]}" for r in sorted(excluded)))


def _slab(mode, Tr, Te, seed, pad=0.0):
    """B chunks over T_m = T_r + T_e memory steps: 0 unpadded; 1 suffix padding in both parts; 2 padding after its first step up to the
    events (in joint mode the row groups after the first hold no live step until the events begin); 3 interior padding: padding at the
    row-group boundaries 31 / 32 / 63 / 64 and at T_r - 1, one event with exactly one feature equal to the padding value, and -- when
    the padding value is 0.0 -- one with a -0.0 feature (utils.input_mask: a step is padding when ANY feature equals the padding
    value, and -0.0 == 0.0); 4 live at T_m - 1 only; 5 unpadded.  `pad` is the handle's input padding value."""
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((B, Tr, 1)).astype(np.float32)
    ev = rng.standard_normal((B, Te, 5)).astype(np.float32)
    pad = np.float32(pad)
    if Tr:
        raw[1, Tr - max(Tr // 3, 1):] = pad
    if Te:
        ev[1, Te - max(Te // 3, 1):] = pad
    (raw if Tr else ev)[2, 1:] = pad
    for t in (31, 32, 63, 64):
        if t < Tr:
            raw[3, t] = pad
        elif not Tr and t < Te:
            ev[3, t, t % 5] = pad
    if Tr:
        raw[3, Tr - 1] = pad
    if Te:
        ev[3, Te // 2, 2] = pad
        if pad == 0.0:
            ev[3, Te - 1, 4] = -0.0
    last = (ev if Te else raw)[4, -1].copy()
    raw[4] = pad
    ev[4] = pad
    (ev if Te else raw)[4, -1] = last
    return raw, ev


def _x(mode, raw, ev):
    return {"joint": (raw, ev), "raw": raw, "event": ev}[mode]


def _oracle_inputs(mode, raw, ev):
    return (raw if mode != "event" else None), (ev if mode != "raw" else None)


def _handle(rv, mode, attention, D, seed, Tr_max=308, Te_max=90, L=16, max_batch=B, tokenizer=None, pad=0.0, enc_depth=2, end_bias=0.05):
    bc = rv.Basecaller(128, 128, 128, tokenizer or rv.data_loader.nuc_tk, mode, pad, encoder_depth=enc_depth, decoder_depth=D,
                       attention_type=attention, honor_attention_type=True, max_batch=max_batch, max_raw_len=Tr_max,
                       max_event_len=Te_max, max_output_len=L)
    flat = rv.weights.init_weights(bc.cfg, seed=seed, gain=1.5)
    flat["b_fc"][bc.cfg.end_token] = end_bias            # chunks finish at different steps, some run all L - 1
    bc.set_weights_flat(flat)
    return bc, rv.weights.flat_to_nested(bc.cfg, flat)


def _set(bc, opts):
    for k, v in opts.items():
        bc.set_option(k, v)


def _decode_forms(bc):
    return {r for r in _rows(bc, "kernel_forms") if r[0] in DECODE}


def _beam(bc, x, W, L, Tm, persist, V=V, B=B):
    """One beam search and its taps (V: the handle's vocabulary, B: the slab's chunks)."""
    tok, sc = bc.beam_search_prediction(x, W, L)
    tok, sc = tok.numpy().copy(), sc.numpy().copy()
    S = tok.shape[1]
    t = lambda name, *shape: bc.get_tensor(name).reshape(shape or (-1,))
    return dict(forms=_decode_forms(bc), tok=tok, sc=sc, cs=t("chunk_steps").astype(int) if persist else np.full(B, S),
                lg=t("step_logits", S, B, W, V), ids=t("step_ids", S, B, W).astype(int), par=t("parent_ids", S, B, W).astype(int),
                al=t("step_alignments", S, B, W, Tm), mask=t("mask", B, Tm))


def _check_beam(oracle, r, o, otok, osc, W, end, tag, twin, B=B):
    """A beam search against the fp64 decode of its slab: the mask exact; on every step where the beams still agree (_agreeing_steps)
    logits within 1e-4 and alignments by _check_alignments; a chunk whose beam ids or parents leave the fp64 decode sits on a genuine
    near-tie; the other chunks' tokens equal the oracle's and their scores are within 1e-4; and logits, alignments and scores no
    further from fp64 than the numpy fp32 twin's (`twin`: test_parity_gpu._twin_beam of the same oracle pass; _assert_twin).  Returns
    the agreeing steps and the chunks that left."""
    assert (r["mask"] == o["mask"]).all(), (tag, "mask")
    So = o["step_ids"].shape[0]
    n = _agreeing_steps(r["ids"], r["par"], o["step_ids"], o["parent_ids"], r["cs"])
    left = set()
    for b in range(B):
        m = min(int(r["cs"][b]), So)
        if ((r["ids"][:m, b] != o["step_ids"][:m, b]) | (r["par"][:m, b] != o["parent_ids"][:m, b])).any():
            gap = _near_tie_gap(oracle, o["step_logits"][:, b], W, end)
            assert gap < TOL, (tag, b, "left the fp64 decode with no near-tie", int(n[b]), gap)
            left.add(b)
        if n[b]:
            assert np.abs(r["lg"][:n[b], b] - o["step_logits"][:n[b], b]).max() < TOL, (tag, b, "step logits")
    _check_alignments(r["al"], o["step_alignments"], o["mask"], r["cs"], tag, last=n)
    if not left:
        assert r["tok"].shape == otok.shape, (tag, r["tok"].shape, otok.shape)
    stay = [b for b in range(B) if b not in left]
    S = min(r["tok"].shape[1], otok.shape[1])
    assert (r["tok"][stay, :S] == otok[stay, :S]).all(), (tag, "tokens")
    assert np.abs(r["sc"][stay, :S] - osc[stay, :S]).max(initial=0.0) < TOL, (tag, "scores")
    err, left_ = _beam_errors(r["lg"], r["al"], r["ids"], r["par"], r["cs"], r["sc"], o, osc)
    assert set(left_) == left, (tag, left_, left)
    _assert_twin(err, twin, tag)
    return n, left


def _check_forms_agree(ref, r, tag):
    """Two forms of one family on the same slab: chunk_steps equal, logits and alignments within 2e-5 on every step both agree with
    the fp64 decode (a chunk that left it at a near-tie in either form is compared up to that step)."""
    (a, na, la), (b_, nb, lb) = ref, r
    for b in range(B):
        if b not in la and b not in lb:
            assert a["cs"][b] == b_["cs"][b], (tag, b, "chunk_steps", a["cs"][b], b_["cs"][b])
        k = min(na[b], nb[b])
        if k:
            assert np.abs(a["lg"][:k, b] - b_["lg"][:k, b]).max() < FORM_TOL, (tag, b, "logits between forms")
            assert np.abs(a["al"][:k, b] - b_["al"][:k, b]).max() < FORM_TOL, (tag, b, "alignments between forms")


def _check_greedy(bc, x, L, Tm, og, olg, gtaps, tag, twin):
    """A greedy search against the fp64 greedy decode: logits within 1e-4 and alignments by _check_alignments up to a chunk's first
    token that differs, which must sit on a genuine near-tie of the fp64 logits; tokens equal otherwise; both no further from fp64
    than the numpy fp32 twin's (`twin`: test_parity_gpu._twin_greedy of the same oracle pass).  Returns the decode forms."""
    tok, lg = bc.greedy_search_prediction(x, L)
    tok, lg = tok.numpy(), lg.numpy()
    S = tok.shape[1]
    al = bc.get_tensor("step_alignments").reshape(S, B, 1, Tm)
    n = np.full(B, min(S, og.shape[1]))
    flipped = False
    for b in range(B):
        diff = np.nonzero(tok[b, :n[b]] != og[b, :n[b]])[0]
        if diff.size:
            n[b] = diff[0] + 1
            top = np.sort(olg[b, n[b] - 1])[::-1]
            assert top[0] - top[1] < TOL, (tag, b, "greedy token differs with no near-tie", top[0] - top[1])
            flipped = True
        assert np.abs(lg[b, :n[b]] - olg[b, :n[b]]).max() < TOL, (tag, b, "greedy logits")
    if not flipped:
        assert tok.shape == og.shape, (tag, tok.shape, og.shape)
    _check_alignments(al, gtaps["step_alignments"][:, :, None], gtaps["mask"], np.full(B, S), tag, last=n)
    _assert_twin(_greedy_errors(tok, lg, al[:, :, 0], og, olg, gtaps)[0], twin, tag)
    return _decode_forms(bc)


def _band_tm(bands, W, band):
    lo, hi = bands[band]
    return hi if (W + band) % 2 else lo           # the two edges alternate across W


def _split(Tm):
    Te = max(1, min(45, Tm // 8))
    return Tm - Te, Te


@pytest.mark.parametrize("fam", list(PERSIST_FAMILIES))
def test_persistent_decode_forms(rv, oracle, fam):
    """Every k_dec_persist<W, NIT, D, ATT> of one family (persist_taps 1): every beam width at each of the three NIT bands, T_m on the
    bands' edges, plus one raw-mode and one event-mode slab; every ATT of the family on each slab against ONE fp64 oracle pass, and
    the ATT forms against each other; greedy search too at W = 1."""
    attention, D, wmax, atts = PERSIST_FAMILIES[fam]
    cases = [("joint", W, *_split(_band_tm(PERSIST_BANDS, W, nit))) for W in range(1, wmax + 1) for nit in PERSIST_BANDS]
    cases += [("raw", 3, 300, 0), ("event", min(6, wmax), 0, 90)]
    handles, ran = {}, set()
    for i, (mode, W, Tr, Te) in enumerate(cases):
        if mode not in handles:
            handles[mode] = _handle(rv, mode, attention, D, seed=70 + len(handles))
        bc, w = handles[mode]
        bc.set_option("persist_taps", 1)
        cfg = bc.cfg.oracle_cfg()
        end = cfg["end_token"]
        raw, ev = _slab(mode, Tr, Te, seed=1000 + i)
        x, (r_, e_) = _x(mode, raw, ev), _oracle_inputs(mode, raw, ev)
        L, Tm = 14 + W % 3, Tr + Te
        nit = min(k for k in PERSIST_BANDS if Tm <= 32 * k)
        taps = {}
        otok, osc = oracle.beam_search(w, cfg, r_, e_, W, L, dtype=np.float64, taps=taps)
        twin = _twin_beam(oracle, w, cfg, r_, e_, W, L, taps, osc, f"{fam} {mode} W={W} T_m={Tm}")
        if W == 1:
            gtaps = {}
            og, olg = oracle.greedy_search(w, cfg, r_, e_, L, dtype=np.float64, taps=gtaps)
            gtwin = _twin_greedy(oracle, w, cfg, r_, e_, L, og, olg, gtaps, f"{fam} {mode} T_m={Tm} greedy")
        got = {}
        for att, opts in atts.items():
            tag = f"{fam} {mode} W={W} T_m={Tm} ATT={att}"
            _set(bc, opts)
            want = _f(PERSIST, W, nit, D, att)
            r = _beam(bc, x, W, L, Tm, persist=True)
            assert r["forms"] == {want}, (tag, sorted(r["forms"]))
            ran.add(want)
            n, left = _check_beam(oracle, r, taps, otok, osc, W, end, tag, twin)
            got[att] = (r, n, left)
            if W == 1:
                assert _check_greedy(bc, x, L, Tm, og, olg, gtaps, tag + " greedy", gtwin) == {want}, tag
        ref = next(iter(atts))
        for att in atts:
            if att != ref:
                _check_forms_agree(got[ref], got[att], f"{fam} {mode} W={W} T_m={Tm} ATT {ref} vs {att}")
    _assert_family_ran(handles["joint"][0], f"persist:{fam}", ran)
    for bc, _ in handles.values():
        bc.close()


def _taps_off_identical(bc, x, W, L, r, tag):
    """Without debug_taps the per-step kernels take their finished-chunk fast path: tokens and score bits equal the taps-on call's,
    and the forms reported -- at the decode graph's capture and at its replay -- are the taps-on call's."""
    bc.set_option("debug_taps", 0)
    for k in range(2):                                   # capture, replay
        tok, sc = bc.beam_search_prediction(x, W, L)
        assert _decode_forms(bc) == r["forms"], (tag, k, sorted(_decode_forms(bc)))
        assert tok.numpy().shape == r["tok"].shape and (tok.numpy() == r["tok"]).all(), (tag, k)
        assert np.array_equal(sc.numpy().view(np.uint32), r["sc"].view(np.uint32)), (tag, k)
    bc.set_option("debug_taps", 1)


@pytest.mark.parametrize("kind", ["flash", "luong", "bahdanau"])
def test_per_step_attend_forms(rv, oracle, kind):
    """Every reachable attend form of the per-step decode (persistent_decode 0, debug_taps 1): k_dec_attend_flash<W <= 5, NT> at
    attend_threads 256 and 512; k_dec_attend<W, TB> for W 1-8 at each TB band, T_m on the bands' edges, for Luong (flash_attend 0, or
    W > 5) and Bahdanau -- the checks of the persistent decode, and one call per kind without taps."""
    bc, w = _handle(rv, "joint", "bahdanau" if kind == "bahdanau" else "luong", 1, seed=80)
    cfg = bc.cfg.oracle_cfg()
    end = cfg["end_token"]
    _set(bc, dict(persistent_decode=0, debug_taps=1))
    if kind == "flash":
        cases = [(W, (64, 65, 224, 225, 352)[W - 1], [(dict(flash_attend=1, attend_threads=NT), _f(FLASH, W, NT)) for NT in (256, 512)])
                 for W in range(1, 6)]
    else:
        cases = [(W, _band_tm(ATTEND_BANDS, W, tb), [(dict(flash_attend=0 if W <= 5 else 1), _f(ATTEND, W, tb))])
                 for W in range(1, 9) for tb in ATTEND_BANDS]
    ran, fast_path = set(), {"flash": 3, "luong": 7, "bahdanau": 4}[kind]
    for i, (W, Tm, runs) in enumerate(cases):
        Tr, Te = _split(Tm)
        raw, ev = _slab("joint", Tr, Te, seed=2000 + i)
        L = 14 + W % 3
        taps = {}
        otok, osc = oracle.beam_search(w, cfg, raw, ev, W, L, dtype=np.float64, taps=taps)
        twin = _twin_beam(oracle, w, cfg, raw, ev, W, L, taps, osc, f"{kind} W={W} T_m={Tm}")
        for opts, want in runs:
            tag = f"{kind} W={W} T_m={Tm} {opts}"
            _set(bc, opts)
            r = _beam(bc, (raw, ev), W, L, Tm, persist=False)
            assert r["forms"] == {want}, (tag, sorted(r["forms"]))
            ran.add(want)
            _check_beam(oracle, r, taps, otok, osc, W, end, tag, twin)
            if W == fast_path:
                _taps_off_identical(bc, (raw, ev), W, L, r, tag)
                fast_path = None
    _assert_family_ran(bc, "flash" if kind == "flash" else "attend", ran)
    bc.close()


# (attention, decoder cells, beam or "greedy"): what the persistent decode hands to the per-step kernels
HANDED_OVER = [("luong", D, W) for D in (3, 4) for W in (1, 5, 8, "greedy")] + \
              [("bahdanau", 2, 3), ("bahdanau", 2, "greedy"), ("luong", 2, 6), ("luong", 2, 7), ("luong", 2, 8)]


@pytest.mark.parametrize("attention,D", sorted({(a, D) for a, D, _ in HANDED_OVER}))
def test_per_step_decode_of_what_the_persistent_decode_hands_over(rv, oracle, attention, D):
    """Three and four decoder cells (k_dec_cell at layers 2 and 3), Bahdanau with two cells, two cells at beams 6-8: the per-step
    kernels with debug_taps against fp64, and each configuration without taps (persistent_decode left on): it does hand over (no
    k_dec_persist), and its tokens and score bits equal the taps-on call's."""
    bc, w = _handle(rv, "joint", attention, D, seed=90 + D)
    cfg = bc.cfg.oracle_cfg()
    end = cfg["end_token"]
    Tr, Te = 60, 12
    Tm = Tr + Te
    raw, ev = _slab("joint", Tr, Te, seed=3000 + D)
    for W in [W for a, D_, W in HANDED_OVER if (a, D_) == (attention, D)]:
        tag = f"{attention} D={D} W={W}"
        Wd = 1 if W == "greedy" else W                  # the effective beam
        L = 14 + Wd % 3
        want = _f(FLASH, Wd, 512) if attention == "luong" and Wd <= 5 else _f(ATTEND, Wd, 7)     # (T_m 72: TB 7; B <= 320: NT 512)
        bc.set_option("debug_taps", 1)
        if W == "greedy":
            gtaps = {}
            og, olg = oracle.greedy_search(w, cfg, raw, ev, L, dtype=np.float64, taps=gtaps)
            gtwin = _twin_greedy(oracle, w, cfg, raw, ev, L, og, olg, gtaps, tag)
            assert _check_greedy(bc, (raw, ev), L, Tm, og, olg, gtaps, tag, gtwin) == {want}, tag
            tok, lg = bc.greedy_search_prediction((raw, ev), L)
            bc.set_option("debug_taps", 0)
            tok2, lg2 = bc.greedy_search_prediction((raw, ev), L)
            assert _decode_forms(bc) == {want}, (tag, sorted(_decode_forms(bc)))
            assert (tok2.numpy() == tok.numpy()).all() and np.array_equal(lg2.numpy().view(np.uint32), lg.numpy().view(np.uint32)), tag
            continue
        taps = {}
        otok, osc = oracle.beam_search(w, cfg, raw, ev, W, L, dtype=np.float64, taps=taps)
        r = _beam(bc, (raw, ev), W, L, Tm, persist=False)
        assert r["forms"] == {want}, (tag, sorted(r["forms"]))
        _check_beam(oracle, r, taps, otok, osc, W, end, tag, _twin_beam(oracle, w, cfg, raw, ev, W, L, taps, osc, tag))
        _taps_off_identical(bc, (raw, ev), W, L, r, tag)
    bc.close()


def _interior_padding(raw, ev, rng):
    """Interior padding in every fifth chunk (from chunk 3): raw zeros at the row-group boundaries and at T_r - 1, an event with one
    zero feature, an event with a -0.0 feature (the feature turns over from chunk to chunk); every eleventh chunk (from 4) padding
    after its first raw step."""
    Tr, Te = raw.shape[1], ev.shape[1]
    for b in range(3, raw.shape[0], 5):
        raw[b, [31, 32, 63, 64, Tr - 1]] = 0.0
        ev[b, rng.integers(0, Te), (b // 5) % 5] = 0.0
        ev[b, rng.integers(0, Te), (b // 5 + 2) % 5] = -0.0
    raw[4::11, 1:] = 0.0


# chunks per workgroup of the packed-FMA kernels (pick_rows_per_block: ~256 workgroups over both directions, a power of two <= 8)
FMA_BT = {97: 1, 200: 2, 387: 4, 1000: 8}
FMA_OPTS = [dict(tail_wave=1, fused_projection=1, split_projection=2), dict(tail_wave=0, fused_projection=1, split_projection=0),
            dict(tail_wave=1, fused_projection=1, split_projection=1), dict(tail_wave=0, fused_projection=0, split_projection=2)]
MX_OPTS = [dict(wide_recurrence=wide, lane_projection=lane) for wide in (1, 2) for lane in (1, 0)]
MX_B = (97, 387)                                     # neither a multiple of 8 nor of 16: a partial last workgroup in both matrix forms


def _encoder_forms(B_, opts):
    if opts.get("wide_recurrence", 1) == 0:
        bt = FMA_BT[B_]
        l0 = lambda F: _f(REC_TW, bt, F) if opts["tail_wave"] and bt >= 2 else _f(REC, bt, F)
        return {l0(1), l0(5), _f(REC_PROJ, bt, opts["split_projection"]) if opts["fused_projection"] else _f(REC, bt, 0)}
    ch = 16 if opts["wide_recurrence"] == 1 else 8
    ev0 = {_f(REC_MX, 5, ch)} if opts["lane_projection"] else {_f(INPROJ, 5), _f(REC_MX, 0, ch)}
    return {_f(REC_MX, 1, ch), _f(REC_MX, 0, ch)} | ev0


def test_encoder_recurrence_forms(rv, oracle):
    """Every recurrence form, joint mode, two encoder layers, T_r 90 / T_e 15: the packed-FMA kernels (wide_recurrence 0) at B = 97 /
    200 / 387 / 1000 (one / two / four / eight chunks per workgroup, a partial last workgroup) with tail_wave 1 and 0, fused_projection 0,
    and fused_projection 1 x split_projection 0 / 1 / 2 -- tail_wave 0 is the only way to k_lstm_rec<BT >= 2, 1 | 5>: the fallback of
    launch_lstm_rec to it never fires inside the library's limits (at eight chunks per workgroup tw_lds_bytes stays under 160 KB up to
    896 event steps and 4,480 raw steps); the matrix-pipe forms (wide_recurrence 1 and 2 x lane_projection 1 / 0) at B = 97 and 387.
    enc_output within 1e-4 of fp64 on chunk 0, the last chunk and the first and last chunk of a middle workgroup of each form; the
    forms of one B within 2e-5 of each other; the mask exactly the oracle's from every writer (k_input_mask, the in-lane writers of
    k_lstm_rec_mx<1 | 5, CH>, k_inproj_small<5>) on interior padding, -0.0 and single zero features."""
    Tr, Te = 90, 15
    Tm = Tr + Te
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=2, max_batch=1000, max_raw_len=Tr,
                       max_event_len=Te, max_output_len=2)
    flat = bc.init_random_weights(seed=41)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    ran = set()
    for Bn in FMA_BT:
        raw, ev, _ = rv.synthetic.make_slab(Bn, Tr, Te, seed=Bn)
        _interior_padding(raw, ev, np.random.default_rng(Bn))
        omask = np.concatenate([oracle.input_mask(raw), oracle.input_mask(ev)], axis=1)
        configs = [dict(wide_recurrence=0, lane_projection=1, **o) for o in FMA_OPTS]
        if Bn in MX_B:
            configs += [dict(tail_wave=1, fused_projection=1, split_projection=2, **o) for o in MX_OPTS]
        groups = {FMA_BT[Bn]} | ({8, 16} if Bn in MX_B else set())
        sample = {0, Bn - 1}
        for G in groups:
            g = (Bn + G - 1) // G // 2
            sample |= {g * G, min(g * G + G - 1, Bn - 1)}
        sample = sorted(sample)
        o_enc, _ = oracle.encode_input(w, raw[sample], ev[sample], "joint", 0.0, np.float64)
        t_enc, _ = oracle.encode_input(w, raw[sample], ev[sample], "joint", 0.0, np.float32)
        twin = dict(enc_output=float(np.abs(t_enc - o_enc).max()))
        ref = None
        for opts in configs:
            tag = f"B={Bn} {opts}"
            _set(bc, opts)
            bc.beam_search_prediction((raw, ev), 1, 2)
            forms = {r for r in _rows(bc, "kernel_forms") if r[0] in ENCODER}
            assert forms == _encoder_forms(Bn, opts), (tag, sorted(forms))
            ran |= forms
            assert (bc.get_tensor("mask").reshape(Bn, Tm) == omask).all(), (tag, "mask")
            enc = bc.get_tensor("enc_output").reshape(Bn, Tm, 256)
            err = float(np.abs(enc[sample] - o_enc).max())
            assert err < TOL, (tag, "enc_output vs fp64", err)
            _assert_twin(dict(enc_output=err), twin, "recurrence " + tag)
            if ref is None:
                ref = enc
            else:
                assert np.abs(enc - ref).max() < FORM_TOL, (tag, "enc_output between forms", float(np.abs(enc - ref).max()))
    for fam in ("fma", "mx"):
        _assert_family_ran(bc, fam, ran)
    bc.close()


def test_every_listed_form_has_a_family(rv):
    """kernel_form_list: each listed form belongs to exactly one of the families the tests above cover, and the exclusions are listed
    forms -- a form or a kernel added to a list without a test fails here or in its family's test."""
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, max_batch=4)
    rows = _rows(bc, "kernel_form_list")
    bc.close()
    orphans = sorted(r for r in rows if _family(r) not in FAMILIES)
    assert not orphans, f"listed forms no test covers: {orphans}"
    assert set(EXCLUDED) <= rows, sorted(set(EXCLUDED) - rows)
    for fam in FAMILIES:
        n = sum(_family(r) == fam for r in rows)
        print(f"{fam}: {n} listed, {sum(_family(r) == fam for r in EXCLUDED)} excluded")
