"""Option fused_inproj: BiLSTM layers >= 1 of a sixteen-chunk matrix-pipe call project their own inputs (csrc/lstm_mx.hip:
k_lstm_rec_mx_proj) instead of reading xw [B,T,2,512] from the split GEMM (k_gemm_ws).  The kernel keeps the GEMM's chain per element
and the recurrence's step, so nothing downstream may move by a bit.  Held here, with fused_inproj = 0 (the two launches) as the
reference on the same handle and inputs:

* enc_output, tokens, score bits and chunk_steps are identical byte for byte at 1 / 15 / 16 / 17 / 33 chunks (an all-copy tail of a
  workgroup, a second workgroup with one live chunk), raw lengths 1 .. 7 and 31 (every pair-plus-remainder case in both directions, the
  first pass with nothing requested ahead, the fragment buffers' wrap), event lengths 1, 2, 3, 30, in every mode, encoder depth 2 and 3;
* with weight_parts 1; with input-kernel columns scaled by 2^10 / 2^-10 and one outlier weight; with layer 0 saturated (|act| at 1);
* three asynchronous slabs of 20, 7 and 21 chunks coalesced into one group (group_inplace 0 and 1) return each slab's synchronous
  result, and the group ran the projecting form;
* the forms are accounted for under a kernel id and a list of their own; kernel_form_list is what it was;
* the per-call choice (-1, the default) runs the form its rule states, with the same results: a small synchronous call keeps the two
  launches; ten slabs in flight take the projecting form at 128 chunks each (1,280 in flight) and not at 127, as single submits and
  coalesced three to a group, where the group's first member decides;
* under `profile` 1 no `gemm_inproj_*` scope runs with the option at 1;
* an explicit 1 is refused by name on a bigru handle and with wide_recurrence 0 or 2, and leaves the handle as it was;
* one joint slab through the fp64 oracle with the option at 1 (a guard in case both paths are ever changed together)."""
import numpy as np
import pytest

from test_kernel_forms_gpu import TOL, _assert_twin, _slab as _kf_slab

L = 8
K_REC_MX = 6                 # csrc/common.h: RV_K_LSTM_REC_MX
K_REC_MX_PROJ = 12           # RV_K_LSTM_REC_MX_PROJ
FUSED_MIN_CHUNKS = 1280      # csrc/ravvent_hip.cpp: FUSED_INPROJ_MIN_CHUNKS, the -1 rule

# (chunks, mode, T_r, T_e, encoder depth)
CASES = [(1, "raw", 1, 0, 2), (15, "raw", 2, 0, 2), (16, "raw", 3, 0, 3), (17, "raw", 4, 0, 2), (33, "raw", 5, 0, 2),
         (17, "raw", 6, 0, 3), (33, "raw", 7, 0, 2), (17, "raw", 31, 0, 2), (33, "event", 0, 1, 2), (17, "event", 0, 2, 2),
         (15, "event", 0, 3, 3), (16, "event", 0, 30, 2), (33, "joint", 31, 30, 2), (17, "joint", 7, 3, 3), (1, "joint", 5, 2, 2),
         (16, "joint", 6, 1, 2)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _mk(rv, mode, Tr, Te, depth, max_batch, seed=11, edit=None, rnn="bilstm"):
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=depth, rnn_type=rnn, max_batch=max_batch,
                       max_raw_len=max(Tr, 1), max_event_len=max(Te, 1), max_output_len=L)
    flat = rv.weights.init_weights(bc.cfg, seed=seed, gain=1.5)
    flat["b_fc"][bc.cfg.end_token] = 0.2
    if edit:
        edit(flat)
    bc.set_weights_flat(flat)
    return bc


def _input(rv, mode, Bn, Tr, Te, seed):
    raw, ev, _ = rv.synthetic.make_slab(Bn, max(Tr, 1), max(Te, 1), seed=seed, max_raw_pad=min(3, max(Tr - 1, 0)),
                                        max_event_pad=min(3, max(Te - 1, 0)))
    return {"joint": (raw, ev), "raw": raw, "event": ev}[mode]


def _rows(bc, name):
    return [tuple(int(v) for v in r) for r in bc.get_tensor(name).reshape(-1, 5)]


def _run(bc, x, Bn, Tm):
    t, s = bc.beam_search_prediction(x, 5, L)
    return (t.numpy().copy(), s.numpy().copy(), bc.get_tensor("chunk_steps").astype(int).copy(),
            bc.get_tensor("enc_output").reshape(Bn, Tm, 256).copy())


def _both(bc, x, Bn, Tm, tag):
    """The call with the option at 0 and at 1: identical outputs; the forms each ran.  Returns the reference outputs."""
    got = {}
    for fused in (0, 1):
        bc.set_option("fused_inproj", fused)
        got[fused] = _run(bc, x, Bn, Tm)
        ids = {r[0] for r in _rows(bc, "kernel_forms")}
        assert (K_REC_MX_PROJ in ids) == (fused == 1), (tag, fused, sorted(ids))
        if fused:
            assert (K_REC_MX, 0, 16, 0, 0) not in _rows(bc, "kernel_forms"), (tag, "the pre-projected form ran beside the projecting one")
    for name, a, b in zip(("tokens", "scores", "chunk_steps", "enc_output"), got[1], got[0]):
        bad = np.argwhere(_bits(a) != _bits(b))
        assert bad.size == 0, f"{tag} {name}: {len(bad)} of {a.size} values differ, first {bad[:4].tolist()}"
    assert np.isfinite(got[0][3]).all() and np.abs(got[0][3]).max() > 1e-3, tag      # a real encoder output, not an untouched buffer
    return got[0]


@pytest.mark.gpu
@pytest.mark.parametrize("Bn,mode,Tr,Te,depth", CASES, ids=[f"B{b}-{m}-{r}+{e}-d{d}" for b, m, r, e, d in CASES])
def test_projecting_form_is_the_two_launches_bit_for_bit(rv, Bn, mode, Tr, Te, depth):
    bc = _mk(rv, mode, Tr, Te, depth, Bn, seed=11 + Bn + Tr + Te)
    _both(bc, _input(rv, mode, Bn, Tr, Te, seed=Bn + 7 * Tr + Te), Bn, Tr + Te, f"B={Bn} {mode} {Tr}+{Te} depth {depth}")
    bc.close()


def _scaled_columns(flat):
    """The column-factor cases of test_split_projection_is_as_close_to_fp64_as_the_f32_mfma: columns of the layer-1 input kernels times
    2^10 and 2^-10, and one outlier weight."""
    for enc in ("raw", "event"):
        for dr in ("fwd", "bwd"):
            W = flat[f"enc_{enc}.1.{dr}.W"]
            W[:, 5:40] *= 2.0 ** 10
            W[:, 200:260] *= 2.0 ** -10
            W[17, 300] = 3.0


def _saturated(flat):
    """Layer 0 driven into saturation: |act| at its bound 1 (c grows with the forget gate open, o open)."""
    for k in flat:
        if k.startswith("enc_") and ".0." in k and k.endswith(".b"):
            flat[k][:] = 12.0
        if k.startswith("enc_") and ".0." in k and k.endswith(".W"):
            flat[k] *= 8.0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["weight_parts_1", "scaled_columns", "saturated_layer0"])
def test_special_weights(rv, kind):
    Bn, mode, Tr, Te = 17, "joint", 31, 7
    edit = {"scaled_columns": _scaled_columns, "saturated_layer0": _saturated}.get(kind)
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, encoder_depth=2, max_batch=Bn, max_raw_len=Tr, max_event_len=Te,
                       max_output_len=L)
    if kind == "weight_parts_1":
        bc.set_option("weight_parts", 1)
    flat = rv.weights.init_weights(bc.cfg, seed=3, gain=1.5)
    flat["b_fc"][bc.cfg.end_token] = 0.2
    if edit:
        edit(flat)
    bc.set_weights_flat(flat)
    ref = _both(bc, _input(rv, mode, Bn, Tr, Te, seed=5), Bn, Tr + Te, kind)
    if kind == "saturated_layer0":
        assert np.abs(ref[3]).max() <= 1.0
    bc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [0, 1])
def test_coalesced_group_straddling_workgroups(rv, inplace):
    import torch
    mode, Tr, Te = "joint", 31, 7
    sizes = (20, 7, 21)
    bc = _mk(rv, mode, Tr, Te, 2, max(sizes), seed=9)
    slabs = [_input(rv, mode, n, Tr, Te, seed=40 + n) for n in sizes]
    bc.set_option("fused_inproj", 0)
    want = [_run(bc, x, n, Tr + Te) for x, n in zip(slabs, sizes)]
    bc.set_async_depth(3)
    bc.set_option("coalesce", 3)
    bc.set_option("group_inplace", inplace)
    bc.set_option("fused_inproj", 1)
    dev = [tuple(torch.from_numpy(a).cuda() for a in x) for x in slabs]
    outs = list(bc.beam_search_stream(dev, 5, L))
    assert len(outs) == 3
    for k, (t, s) in enumerate(outs):
        assert (t.cpu().numpy() == want[k][0]).all() and _same(s.cpu().numpy(), want[k][1]), (inplace, k)
    stats = bc.get_tensor("coalesce_stats")
    assert stats[0] >= 1 and stats[2] == 3, stats
    rows = _rows(bc, "group_kernel_forms")
    assert (K_REC_MX_PROJ, 16, 0, 0, 0) in rows and (K_REC_MX, 0, 16, 0, 0) not in rows, rows
    bc.close()


@pytest.mark.gpu
def test_form_accounting_and_per_call_rule(rv):
    Bn, mode, Tr, Te = 17, "joint", 7, 3
    bc = _mk(rv, mode, Tr, Te, 2, Bn, seed=2)
    listed = _rows(bc, "kernel_form_list")
    assert all(r[0] != K_REC_MX_PROJ for r in listed) and (K_REC_MX, 0, 16, 0, 0) in listed
    assert _rows(bc, "kernel_form_list_proj") == [(K_REC_MX_PROJ, 16, 0, 0, 0)]
    x = _input(rv, mode, Bn, Tr, Te, seed=1)
    ref = _both(bc, x, Bn, Tr + Te, "accounting")
    assert (K_REC_MX_PROJ, 16, 0, 0, 0) in _rows(bc, "kernel_forms")      # every form of the new list ran
    assert _rows(bc, "kernel_form_list") == listed
    # the per-call rule: fewer than FUSED_MIN_CHUNKS chunks in flight keep the two launches
    bc.set_option("fused_inproj", -1)
    got = _run(bc, x, Bn, Tr + Te)
    ids = {r[0] for r in _rows(bc, "kernel_forms")}
    assert (K_REC_MX_PROJ in ids) == (Bn >= FUSED_MIN_CHUNKS), sorted(ids)
    for a, b in zip(got, ref):
        assert _same(a, b)
    bc.close()


def _stream_case(rv, sizes, coalesce, depth=10, n_slabs=10):
    """Slabs of `sizes` chunks (cycled to n_slabs) through the asynchronous calls at `depth` under the DEFAULT option (-1), against the
    synchronous calls with the option at 0.  Returns the rows of kernel_forms (single submits: slot 0's last call) or of
    group_kernel_forms (coalesced)."""
    import warnings
    import torch
    mode, Tr, Te = "joint", 7, 3
    bc = _mk(rv, mode, Tr, Te, 2, max(sizes), seed=4)
    slabs = [_input(rv, mode, n, Tr, Te, seed=60 + n + k) for k, n in enumerate(sizes)]
    bc.set_option("fused_inproj", 0)
    want = [_run(bc, x, n, Tr + Te) for x, n in zip(slabs, sizes)]
    bc.set_option("fused_inproj", -1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (more contexts than hardware queues: a warning, the option takes effect)
        bc.set_async_depth(depth)
    bc.set_option("coalesce", coalesce)
    dev = [tuple(torch.from_numpy(a).cuda() for a in x) for x in slabs]
    order = [k % len(sizes) for k in range(n_slabs)]
    outs = list(bc.beam_search_stream([dev[k] for k in order], 5, L))
    assert len(outs) == n_slabs
    for k, (t, s) in zip(order, outs):
        assert (t.cpu().numpy() == want[k][0]).all() and _same(s.cpu().numpy(), want[k][1]), (sizes, coalesce, k)
    if coalesce >= 2:
        assert bc.get_tensor("coalesce_stats")[0] >= 1
    rows = _rows(bc, "group_kernel_forms" if coalesce >= 2 else "kernel_forms")
    bc.close()
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("first,fused", [(128, True), (127, False)], ids=["1280-in-flight", "1270-in-flight"])
def test_default_rule_single_submits(rv, first, fused):
    """Option at its default (-1), ten slabs in flight, one context each: `first` chunks x depth 10 on either side of the rule's 1,280."""
    assert (first * 10 >= FUSED_MIN_CHUNKS) == fused
    rows = _stream_case(rv, (first,) * 3, coalesce=0)
    assert ((K_REC_MX_PROJ, 16, 0, 0, 0) in rows) == fused, rows
    assert ((K_REC_MX, 0, 16, 0, 0) in rows) == (not fused), rows


@pytest.mark.gpu
@pytest.mark.parametrize("sizes,fused", [((128, 7, 21), True), ((127, 128, 128), False)], ids=["first-member-128", "first-member-127"])
def test_default_rule_coalesced_group(rv, sizes, fused):
    """... and coalesced three to a group: the rule takes the group's FIRST member's chunks x depth, whatever the others hold."""
    assert (sizes[0] * 10 >= FUSED_MIN_CHUNKS) == fused
    rows = _stream_case(rv, sizes, coalesce=3, n_slabs=9)
    assert ((K_REC_MX_PROJ, 16, 0, 0, 0) in rows) == fused, rows
    assert ((K_REC_MX, 0, 16, 0, 0) in rows) == (not fused), rows


@pytest.mark.gpu
def test_no_projection_launch_under_the_option(rv):
    """`profile` 1: with the option at 1 no `gemm_inproj_*` scope runs and the `lstm_rec_*_l1p` scopes do; at 0 both run."""
    Bn, mode, Tr, Te = 17, "joint", 7, 3
    bc = _mk(rv, mode, Tr, Te, 3, Bn, seed=6)
    x = _input(rv, mode, Bn, Tr, Te, seed=2)
    bc.set_option("profile", 1)
    for fused in (0, 1):
        bc.set_option("fused_inproj", fused)
        bc.reset_profile()
        bc.beam_search_prediction(x, 5, L)
        names = set(bc.profile())
        assert {"lstm_rec_raw_l1p", "lstm_rec_event_l1p"} <= names, (fused, names)
        assert ({"gemm_inproj_raw", "gemm_inproj_event"} <= names) == (fused == 0), (fused, names)
        assert not (fused and any(n.startswith("gemm_inproj") for n in names)), names
    bc.close()


@pytest.mark.gpu
def test_refusals_leave_the_handle_as_it_was(rv):
    mode, Tr, Te, Bn = "joint", 7, 3, 5
    gru = _mk(rv, mode, Tr, Te, 2, Bn, rnn="bigru")
    x = _input(rv, mode, Bn, Tr, Te, seed=1)
    before = gru.beam_search_prediction(x, 5, L)
    with pytest.raises(Exception, match="fused_inproj"):
        gru.set_option("fused_inproj", 1)
    after = gru.beam_search_prediction(x, 5, L)
    assert (before[0].numpy() == after[0].numpy()).all() and _same(before[1].numpy(), after[1].numpy())
    gru.close()
    bc = _mk(rv, mode, Tr, Te, 2, Bn)
    for wide in (0, 2):
        bc.set_option("wide_recurrence", wide)
        with pytest.raises(Exception, match="fused_inproj"):
            bc.set_option("fused_inproj", 1)
        bc.beam_search_prediction(x, 5, L)
        assert all(r[0] != K_REC_MX_PROJ for r in _rows(bc, "kernel_forms")), wide
    bc.set_option("wide_recurrence", 1)
    bc.set_option("fused_inproj", 1)
    with pytest.raises(Exception, match="fused_inproj"):
        bc.set_option("wide_recurrence", 2)
    bc.beam_search_prediction(x, 5, L)
    assert any(r[0] == K_REC_MX_PROJ for r in _rows(bc, "kernel_forms"))
    bc.close()


@pytest.mark.gpu
def test_projecting_form_against_fp64(rv, oracle):
    """B 6, 40 + 8 (the slab of test_kernel_forms_gpu._slab) with the option at 1: enc_output within 1e-4 of fp64 and no further from
    it than the numpy fp32 twin allows -- that file's tolerances for the matrix-pipe recurrence."""
    Tr, Te = 40, 8
    raw, ev = _kf_slab("joint", Tr, Te, seed=3)
    Bn = raw.shape[0]
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=2, max_batch=Bn, max_raw_len=Tr, max_event_len=Te,
                       max_output_len=2)
    flat = bc.init_random_weights(seed=41)
    w = rv.weights.flat_to_nested(bc.cfg, flat)
    bc.set_option("fused_inproj", 1)
    bc.beam_search_prediction((raw, ev), 1, 2)
    assert any(r[0] == K_REC_MX_PROJ for r in _rows(bc, "kernel_forms"))
    enc = bc.get_tensor("enc_output").reshape(Bn, Tr + Te, 256)
    o_enc, _ = oracle.encode_input(w, raw, ev, "joint", 0.0, np.float64)
    t_enc, _ = oracle.encode_input(w, raw, ev, "joint", 0.0, np.float32)
    err = float(np.abs(enc - o_enc).max())
    print("enc_output vs fp64:", err, "twin:", float(np.abs(t_enc - o_enc).max()))
    assert err < TOL, err
    _assert_twin(dict(enc_output=err), dict(enc_output=float(np.abs(t_enc - o_enc).max())), "fused_inproj")
    bc.close()
