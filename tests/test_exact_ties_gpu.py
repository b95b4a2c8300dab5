"""Every decode form's beam step held to the exact tie rule of tf.math.top_k: the integer model of test_exact_ties.py (its docstring
has the construction: W_fc = 0, b_fc = 0.25 on a token set H and -1.0e4 elsewhere, so that candidates tie exactly in every arithmetic
and the decode is decided by (live steps n, flat index beam * V + token) alone), reproduced by the GPU with nothing excused: no
near-tie allowance, no chunk left out.

Per call (_check): S and chunk_steps are the model's; step_ids and parent_ids equal the model's on every step, identically for the
three chunks; step_scores of slots with equal model keys are bit-identical (the ties were exact on the device) and -inf on dead beams;
step_logits equal b_fc as values in every beam and step; every slot's score is within 1e-4 of n * (-ln|H|) in fp64, and logits and
top-1 scores are no further from fp64 than TWIN_K x the oracle's numpy fp32 twin + TWIN_C (test_parity_gpu._assert_twin); the call's
tokens are oracle.gather_tree of the model's records and its scores the bits of slot 0.

Shapes: three different chunks (one with suffix padding), T_r 40 + T_e 8 -- the tie logic does not depend on the memory band, so one
band (k_dec_persist NIT 2, k_dec_attend TB 2) is enough -- L 12, max_batch 3.  decode_split only splits slabs of 64 chunks or more and
lays its records out per sub-slab, so its case runs the three chunks tiled to 64 and compares the all-beams outputs."""
import numpy as np
import pytest

from test_beams_gpu import _assert_equal, _expect, _np_beams
from test_config_space_gpu import CONFIGS as SPACE_CONFIGS, PERSIST_ON, PER_STEP, _Tokenizer, _runs
from test_exact_ties import (ALL, B, CONFIGS, HOLES, L, TE, TR, assert_records, greedy_model, model_scores, tie_flat, tie_model,
                             tie_slab, tokens_of)
from test_kernel_forms_gpu import ATTEND, FLASH, PERSIST, PERSIST_FAMILIES, TOL, _beam, _decode_forms, _f, _handle, _set
from test_parity_gpu import _assert_twin

pytestmark = pytest.mark.gpu

TM = TR + TE
NIT, TB = 2, 2                                        # T_m 48: k_dec_persist NIT 2 (T_m <= 64), k_dec_attend TB 2
DEFAULT_FORM = dict(PERSIST_ON, matrix_attention=1, matrix_cell=1)      # k_dec_persist<W, NIT, 1, ATT 3> with its logits tap
UNTAPPED = dict(DEFAULT_FORM, persist_taps=0)                           # the same as the library runs it by default
NEG_INF_BITS = np.float32(-np.inf).view(np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- handles, weights, models, twins
@pytest.fixture(scope="module")
def world(rv, oracle):
    """get(configuration, attention, cells, H) -> the handle with the tie weights of H loaded, and what goes with it."""
    handles, twins = {}, {}

    def get(name, attention="luong", D=1, H=ALL, max_batch=B):
        key = (name, attention, D, max_batch)
        if key not in handles:
            V, start, end, pad_token, pad = CONFIGS[name]
            if name != "default":
                assert CONFIGS[name] == SPACE_CONFIGS[name], name
            tk = None if name == "default" else _Tokenizer(V, start, end, pad_token)
            bc, _ = _handle(rv, "joint", attention, D, seed=5, Tr_max=TR, Te_max=TE, L=L, max_batch=max_batch, tokenizer=tk, pad=pad)
            assert (bc.cfg.vocab, bc.cfg.start_token, bc.cfg.end_token, bc.cfg.pad_token) == (V, start, end, pad_token)
            raw, ev = tie_slab(rv, pad)
            for a in (raw, ev):
                a.setflags(write=False)
            handles[key] = dict(bc=bc, x=(raw, ev), H="unset", name=name, attention=attention, D=D)
        e = handles[key]
        if e["H"] != H:
            e["flat"] = tie_flat(rv, e["bc"].cfg, H)
            e["bc"].set_weights_flat(e["flat"])
            e["H"] = H
        return e

    def twin(e, W):
        """The model of (e's configuration and H, W), its fp64 scores, and the numpy fp32 twin's errors against them (once per case)."""
        key = (e["name"], e["attention"], e["D"], e["H"], W)
        if key not in twins:
            cfg = e["bc"].cfg
            m = tie_model(cfg.vocab, cfg.end_token, e["H"], W, L)
            want = model_scores(m, cfg.vocab, e["H"])
            t = {}
            _, tsc = oracle.beam_search(rv.weights.flat_to_nested(cfg, e["flat"]), cfg.oracle_cfg(), *e["x"], W, L, dtype=np.float32, taps=t)
            assert_records(t, m, "numpy fp32 twin")
            err = dict(step_logits=float(np.abs(t["step_logits"] - e["flat"]["b_fc"]).max()), scores=float(np.abs(tsc - want[None, :, 0]).max()))
            tok = oracle.gather_tree(m["step_ids"][:, None].astype(np.int32), m["parent_ids"][:, None], [int(m["lengths"].max())], cfg.end_token)
            twins[key] = (m, want, err, t["mask"], tok[:, 0, 0])
        return twins[key]

    get.twin = twin
    yield get
    for e in handles.values():
        e["bc"].close()


def _groups(m, H, V):
    """The sets of slots [S, W] whose model keys are equal: one per n (all live slots when |H| = 1), and the dead beams."""
    n = m["n"]
    if len(tokens_of(V, H)) == 1:
        return [n >= 0], n < 0
    return [n == k for k in np.unique(n[n >= 0])], n < 0


def _check(world, e, r, W, tag, nB=B):
    """One beam search with its taps (test_kernel_forms_gpu._beam) against the model: see the module docstring.  Returns the worst
    |step_scores - fp64|."""
    bc, H = e["bc"], e["H"]
    V = bc.cfg.vocab
    m, want, twin, mask, mtok = world.twin(e, W)
    S = m["S"]
    assert r["tok"].shape == (nB, S), (tag, "S", r["tok"].shape, S)
    assert (r["cs"] == S).all(), (tag, "chunk_steps", r["cs"].tolist(), S)
    assert (r["mask"] == mask).all(), (tag, "mask")
    for k, name in (("ids", "step_ids"), ("par", "parent_ids")):
        bad = np.argwhere(r[k] != m[name][:, None])
        assert not bad.size, (tag, name, "first [step, chunk, slot] that differs", bad[0].tolist(), r[k][bad[0][0], bad[0][1]].tolist(),
                              m[name][bad[0][0]].tolist())
    ss = bc.get_tensor("step_scores").reshape(S, nB, W)
    groups, dead = _groups(m, H, V)
    for g in groups:
        u = np.unique(_bits(ss)[np.broadcast_to(g[:, None], ss.shape)])
        assert u.size == 1, (tag, "scores of equal model keys differ in bits", [hex(v) for v in u])
    assert (_bits(ss)[np.broadcast_to(dead[:, None], ss.shape)] == NEG_INF_BITS).all(), (tag, "a dead beam's score is not -inf")
    assert (r["lg"] == e["flat"]["b_fc"]).all(), (tag, "step_logits are not b_fc", np.argwhere(r["lg"] != e["flat"]["b_fc"])[:3].tolist())
    live = np.broadcast_to(~dead[:, None], ss.shape)
    with np.errstate(invalid="ignore"):                   # -inf - -inf on the dead beams, which `live` leaves out
        err = float(np.abs(ss.astype(np.float64) - want[:, None])[live].max())
    assert err < TOL, (tag, "step_scores vs n * -ln|H| in fp64", err)
    assert np.array_equal(_bits(r["sc"]), _bits(ss[:, :, 0].T)), (tag, "the call's scores are not slot 0 of the records")
    assert (r["tok"] == mtok[None]).all(), (tag, "tokens", r["tok"][0].tolist(), mtok.tolist())
    _assert_twin(dict(step_logits=float(np.abs(r["lg"] - e["flat"]["b_fc"]).max()), scores=float(np.abs(r["sc"] - want[None, :, 0]).max())),
                 twin, tag)
    return err


def _want(want, attention, W, opts):
    """The decode form a run of test_config_space_gpu._runs must launch at T_m 48 (its own expectation is for T_m 82)."""
    if want[0] == PERSIST:
        return _f(PERSIST, W, NIT, want[3], want[4])
    return _f(FLASH, W, 512) if attention == "luong" and W <= 5 and opts["flash_attend"] else _f(ATTEND, W, TB)


def _run(world, e, W, label, opts, want, persist, worst):
    tag = f"{e['name']} H={e['H'] or 'all'} {e['attention']}{e['D']} W={W} {label}"
    _set(e["bc"], opts)
    r = _beam(e["bc"], e["x"], W, L, TM, persist=persist, V=e["bc"].cfg.vocab, B=B)
    assert r["forms"] == {want}, (tag, sorted(r["forms"]))
    worst[label] = max(worst.get(label, 0.0), _check(world, e, r, W, tag))


def _report(what, worst):
    print(f"{what}: worst |step_scores - fp64| per form: " + "; ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---------------------------------------------------------------------------------------------- the default form, every beam width
@pytest.mark.parametrize("name", list(CONFIGS))
def test_default_form_every_beam_width(world, name):
    """k_dec_persist<W, 2, 1, ATT 3> for W = 1 .. 8: every W instance of the persistent beam step; V = 7 leaves lanes free and has the
    -inf fillers at W = 8, V = 8 at W = 8 fills the wave (lane 63 is beam 7's last token: the end token in E)."""
    e, worst = world(name), {}
    for W in range(1, 9):
        _run(world, e, W, "ATT 3", DEFAULT_FORM, _f(PERSIST, W, NIT, 1, 3), True, worst)
    _report(f"{name} {CONFIGS[name]}", worst)


# ---------------------------------------------------------------------------------------------- every other form
FORM_CASES = [("default", "luong1"), ("default", "bahdanau1"), ("default", "luong2"), ("default", "luong4"), ("A", "luong1"), ("A", "bahdanau1")]


@pytest.mark.parametrize("name,fam", FORM_CASES, ids=[f"{c}-{f}" for c, f in FORM_CASES])
def test_every_decode_form(world, name, fam):
    """The forms test_config_space_gpu._runs lists for a family -- the persistent ATT forms, single-pass and two-pass per-step attend
    with use_graph 0 and 1, four cells on the per-step path -- at W 3 / 5 / 8 up to the family's widest beam; under configuration A
    at W = 8 (64 candidates: lane 63 in the per-step kernels' beam step too)."""
    attention, D, wmax = ("luong", 4, 8) if fam == "luong4" else PERSIST_FAMILIES[fam][:3]
    e, worst = world(name, attention, D), {}
    for W in [W for W in (3, 5, 8) if W <= wmax and (name == "default" or W == 8)]:
        for label, opts, want, persist in _runs(attention, D, W):
            _run(world, e, W, label, opts, _want(want, attention, W, opts), persist, worst)
    _report(f"{name} {fam}", worst)


@pytest.mark.parametrize("H", HOLES, ids=lambda H: "".join(map(str, H)))
def test_hole_patterns(world, H):
    """Maxima in non-adjacent lanes, W = 4, one persistent and one per-step form: {1,3,4,6} finishes one beam per step (S = 4),
    {3,4,5,6} never finishes and keeps every parent 0."""
    e, worst = world("default", H=H), {}
    _run(world, e, 4, "ATT 3", DEFAULT_FORM, _f(PERSIST, 4, NIT, 1, 3), True, worst)
    _run(world, e, 4, "two-pass graph 1", dict(PER_STEP, use_graph=1, flash_attend=0), _f(ATTEND, 4, TB), False, worst)
    _report(f"default H={H}", worst)


# ---------------------------------------------------------------------------------------------- the whole beam
@pytest.mark.parametrize("name,W", [("default", 5), ("A", 8), ("E", 8)])
@pytest.mark.parametrize("form", ["persistent", "per_step"])
def test_all_beams(world, oracle, form, name, W):
    """rv_beam_search_all on the model's records: tokens = oracle.gather_tree of them, lengths the model's, and -- with the device's
    own step_scores along the model's back-traces (test_beams_gpu._expect) -- scores, path_scores and log_probs bit for bit;
    log_probs non-increasing in w and bitwise equal where the model keys are equal; slot 0 byte-identical to rv_beam_search."""
    e = world(name)
    bc, end = e["bc"], e["bc"].cfg.end_token
    m, want, _, _, _ = world.twin(e, W)
    S = m["S"]
    _set(bc, UNTAPPED if form == "persistent" else dict(UNTAPPED, persistent_decode=0, decode_split=1))
    tag = f"{name} W={W} {form}"
    got = _np_beams(bc.beam_search_hypotheses(e["x"], W, L))
    assert (PERSIST in {r[0] for r in _decode_forms(bc)}) == (form == "persistent"), (tag, sorted(_decode_forms(bc)))
    assert got.tokens.shape == (B, S, W), (tag, got.tokens.shape, S)
    t = lambda k: bc.get_tensor(k).reshape(S, B, W)
    ids, par, ss = t("step_ids").astype(int), t("parent_ids").astype(int), t("step_scores")
    assert (ids == m["step_ids"][:, None]).all() and (par == m["parent_ids"][:, None]).all(), (tag, "records")
    x = _expect(oracle, np.repeat(m["step_ids"][:, None], B, 1), np.repeat(m["parent_ids"][:, None], B, 1), ss, np.full(B, S), end)
    mtok = oracle.gather_tree(m["step_ids"][:, None].astype(np.int32), m["parent_ids"][:, None], [int(m["lengths"].max())], end)[:, 0]
    assert (x["tokens"] == mtok[None]).all() and (x["lengths"] == m["lengths"][None]).all()
    assert (got.tokens == mtok[None]).all(), (tag, "tokens")
    assert (got.lengths == m["lengths"][None]).all(), (tag, "lengths", got.lengths[0].tolist(), m["lengths"].tolist())
    _assert_equal(got, x, tag)
    lp, n = got.log_probs, m["n"][S - 1]
    assert (lp[:, 1:] <= lp[:, :-1]).all(), (tag, "log_probs increase with w", lp[0].tolist())
    for k in np.unique(n):
        assert np.unique(_bits(lp)[:, n == k]).size == 1, (tag, "log_probs of equal model keys differ in bits", k)
    live = n >= 0
    assert np.abs(lp[:, live] - want[S - 1][None, live]).max() < TOL and (_bits(lp[:, ~live]) == NEG_INF_BITS).all(), (tag, "log_probs")
    tok, sc = bc.beam_search_prediction(e["x"], W, L)
    assert np.ascontiguousarray(got.tokens[:, :, 0]).tobytes() == tok.numpy().tobytes(), (tag, "slot 0 tokens")
    assert np.ascontiguousarray(got.scores[:, :, 0]).tobytes() == sc.numpy().tobytes(), (tag, "slot 0 scores")
    print(f"{tag}: S = {S}, lengths {m['lengths'].tolist()}, hypotheses {[''.join(map(str, mtok[:, w])) for w in range(W)]}")


@pytest.mark.parametrize("W", [3, 5, 8])
def test_decode_split(rv, world, oracle, W):
    """decode_split 2 and 4 (per-step decode, 64 chunks -- smaller slabs are never split): every chunk's hypotheses are the model's,
    and the outputs byte-identical to the unsplit call's; W 3 and 5 run the single-pass attend kernel's beam step, W 8 the two-pass
    kernel's, with the -inf fillers of step 0 (V = 7 < W).  The records of a split call are laid out per sub-slab and rv_get_tensor
    refuses them, which is also how the test knows that the call was split."""
    nB = 64
    e = world("default", max_batch=nB)
    bc, end = e["bc"], e["bc"].cfg.end_token
    m = tie_model(bc.cfg.vocab, end, ALL, W, L)
    want = model_scores(m, bc.cfg.vocab, ALL)
    S, dead = m["S"], m["n"] < 0
    assert dead.any() == (W == 8)
    x = tuple(np.ascontiguousarray(np.tile(a, (22, 1, 1))[:nB]) for a in e["x"])
    mtok = oracle.gather_tree(m["step_ids"][:, None].astype(np.int32), m["parent_ids"][:, None], [int(m["lengths"].max())], end)[:, 0]
    form = _f(FLASH, W, 512) if W <= 5 else _f(ATTEND, W, TB)
    one = None
    for split in (1, 2, 4):
        _set(bc, dict(UNTAPPED, persistent_decode=0, decode_split=split))
        got = _np_beams(bc.beam_search_hypotheses(x, W, L))
        tag = f"W={W} decode_split {split}"
        assert _decode_forms(bc) == {form}, (tag, sorted(_decode_forms(bc)))
        if split > 1:
            with pytest.raises(rv._capi.RavventHipError, match="decode_split"):
                bc.get_tensor("step_ids")
        assert got.tokens.shape == (nB, S, W) and (got.tokens == mtok[None]).all(), (tag, "tokens")
        assert (got.lengths == m["lengths"][None]).all(), (tag, "lengths")
        for s in range(S):
            for k in np.unique(m["n"][s]):                 # n = -1: the dead beams, whose bits must be those of -inf
                u = np.unique(_bits(got.scores[:, s])[:, m["n"][s] == k])
                assert u.size == 1 and (k >= 0 or u[0] == NEG_INF_BITS), (tag, "scores of equal model keys differ in bits", s, k)
        live = np.broadcast_to(~dead[None], got.scores.shape)
        with np.errstate(invalid="ignore"):               # -inf - -inf on the dead beams, which `live` leaves out
            err = float(np.abs(got.scores - want[None])[live].max())
        assert err < TOL, (tag, "scores", err)
        if one is None:
            one = got
        for k in one._fields:
            assert getattr(got, k).tobytes() == getattr(one, k).tobytes(), (tag, k, "differs from decode_split 1")
    bc.set_option("decode_split", 1)


# ---------------------------------------------------------------------------------------------- fused post-processing
@pytest.mark.parametrize("H,W", [(HOLES[1], 4), (ALL, 5)], ids=["3456-W4", "all-W5"])
def test_calls(world, oracle, H, W):
    """rv_beam_search_calls: letters and lengths equal the host form's, probs the host form's within the project's 1e-4, and 1/|H| on
    the best hypothesis's own steps.  On exact ties the shortest hypothesis wins, so a call has letters only when nothing finishes,
    and then every parent is 0: H = {3,4,5,6} at W = 4 calls min(H) eleven times (probs 1/4 at each), while H = all at W = 5 gives
    the fused finalize the records with real parents (one beam finishes per step; slot 0 comes from parent 1 at step 1) and calls
    the empty string (its one own step, the end token, has probability 1/7; the later columns repeat the score: 1)."""
    e = world("default", H=H)
    bc = e["bc"]
    m, *_ = world.twin(e, W)
    S = m["S"]
    _set(bc, UNTAPPED)
    tok, sc = bc.beam_search_prediction(e["x"], W, L)
    assert _decode_forms(bc) == {_f(PERSIST, W, NIT, 1, 3)}, sorted(_decode_forms(bc))
    strings = oracle.tokens_to_nuc_sequences(tok.numpy())
    assert strings == (["A" * (L - 1)] if H is not ALL else [""]) * B, strings
    assert (m["parent_ids"] != 0).any() == (H is ALL)
    bases, probs, lens = bc.beam_search_call_arrays(e["x"], W, L)
    assert bc.last_steps == S and lens.tolist() == [len(s) for s in strings]
    for b in range(B):
        assert bases[b, :lens[b]].tobytes().decode("ascii") == strings[b] and (bases[b, lens[b]:] == 0).all(), b
    host = oracle.calc_prob_logits_beam_search_scores(sc.numpy())
    own = int(m["lengths"][0])                              # the best hypothesis's own steps (its end token included)
    p = 1.0 / len(tokens_of(bc.cfg.vocab, H))
    worst, vs_host = float(np.abs(probs[:, :own] - p).max()), float(np.abs(probs[:, :S] - host).max())
    print(f"calls H={H or 'all'} W={W}: own steps {own}, max |probs - 1/|H|| = {worst:.2e}, max |probs - host form| = {vs_host:.2e}")
    assert worst < TOL and vs_host < TOL, (worst, vs_host)


# ---------------------------------------------------------------------------------------------- greedy
@pytest.mark.parametrize("H", [ALL, *HOLES, (6,)], ids=lambda H: "all" if H is None else "".join(map(str, H)))
def test_greedy(world, H):
    """The sampler rides on the beam step's loop: the first maximum, min(H), at every step, the logits rows b_fc, S = 1 when min(H) is
    the end token and L - 1 otherwise -- persistent and per-step."""
    e = world("default", H=H)
    bc = e["bc"]
    t, S = greedy_model(bc.cfg.vocab, bc.cfg.end_token, H, L)
    for label, opts, want in (("persistent", DEFAULT_FORM, _f(PERSIST, 1, NIT, 1, 3)),
                              ("per-step", dict(PER_STEP, use_graph=1, flash_attend=1), _f(FLASH, 1, 512))):
        _set(bc, opts)
        tok, lg = bc.greedy_search_prediction(e["x"], L)
        tok, lg = tok.numpy(), lg.numpy()
        assert _decode_forms(bc) == {want}, (label, sorted(_decode_forms(bc)))
        assert tok.shape == (B, S) and (tok == t).all(), (label, tok.tolist(), t, S)
        assert lg.shape == (B, S, bc.cfg.vocab) and (lg == e["flat"]["b_fc"]).all(), (label, "logits are not b_fc")


# ---------------------------------------------------------------------------------------------- asynchronous calls, slab graph
def test_async_and_slab_graph(world):
    """One tie slab (configuration A, W = 8) through submit / collect at async_depth 4, coalesce 2 (the slab twice: a group of two),
    and through a slab graph: tokens and score bits of the synchronous call, which _check holds to the model."""
    e, W = world("A"), 8
    bc = e["bc"]
    _set(bc, DEFAULT_FORM)
    r = _beam(bc, e["x"], W, L, TM, persist=True, V=bc.cfg.vocab, B=B)
    _check(world, e, r, W, "A W=8 synchronous")
    _set(bc, UNTAPPED)
    same = lambda got: (got[0].numpy().shape == r["tok"].shape and np.array_equal(got[0].numpy(), r["tok"]) and
                        np.array_equal(_bits(got[1].numpy()), _bits(r["sc"])))
    assert same(bc.beam_search_prediction(e["x"], W, L)), "without taps"
    try:
        bc.set_async_depth(4)
        bc.set_coalesce(2)
        g0, s0 = (int(v) for v in bc.get_tensor("coalesce_stats")[:2])
        tickets = [bc.submit_beam_search(e["x"], W, L) for _ in range(2)]
        for k, t in enumerate(tickets):
            assert same(bc.collect(t)), f"ticket {k} differs from the synchronous call"
        g1, s1 = (int(v) for v in bc.get_tensor("coalesce_stats")[:2])
        assert (g1 - g0, s1 - s0) == (1, 2), ("the two slabs did not run as one group", g1 - g0, s1 - s0)
        bc.set_coalesce(-1)
        bc.set_option("slab_graph", 1)
        for k in range(2):                                   # capture, replay
            assert same(bc.beam_search_prediction(e["x"], W, L)), f"slab_graph call {k} differs from the synchronous call"
    finally:
        bc.set_option("slab_graph", 0)
        bc.set_async_depth(2)
        bc.set_coalesce(-1)
