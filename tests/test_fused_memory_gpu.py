"""Option fused_memory (default 1): the default decode form -- Luong attention, one decoder cell, everything on the matrix pipe,
k_dec_persist<W, NIT, 1, 3> -- projects its chunk's attention memory [keys | U'] = enc_out . [W_mem | A_c] in its own prologue
(csrc/decode.hip: persist_project_memory) instead of reading what a GEMM launch (`gemm_memory`, k_gemm_mem_split3) wrote.  The
prologue keeps the GEMM's chain per element, so nothing downstream may move by a bit.  Held here, with fused_memory = 0 (the GEMM
path) as the reference on the same input and weights:

* the fp32 values the workgroups computed (tap `projected_memory` under persist_taps = 1) equal the GEMM's bit for bit, at every
  memory length where a row tile, a 32-step block or the kernel's NIT changes, with ordinary weights and with the special columns of
  tests/test_split_image.py (scales 2^+-20, a zero column, an outlier, power-of-two maxima) in W_mem and A_c;
* tokens, score bits and chunk_steps are identical with the option on and off, beam 5 and greedy, in every input mode, with a chunk
  that is padding from end to end in the slab, without taps too, and through the asynchronous calls at depth 3 over distinct slabs;
* without taps `projected_memory` is built on request and is the same tensor;
* Bahdanau and two-cell handles still launch the GEMM and the option is a no-op for them.

A CPU test holds the two benchmark-width instantiations of the form to the scratch they compile to at this commit."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_split_image import special_weights

L = 12
B = 3
PAD = 1                      # the chunk that is padding from end to end
K_DEC_PERSIST = 0            # csrc/common.h: RV_K_DEC_PERSIST

# (mode, T_r, T_e): T_m = 1, 15, 16, 17, 33 (row-tile and block edges of the short form), 230, 256 (the last NIT = 8), 257 (the first
# NIT = 11), 330, 352 (the longest memory the decode is built for)
SIZES = [("raw", 1, 0), ("event", 0, 15), ("joint", 11, 5), ("raw", 17, 0), ("joint", 25, 8), ("joint", 200, 30), ("joint", 226, 30),
         ("joint", 227, 30), ("joint", 290, 40), ("joint", 307, 45)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _mk(rv, mode, Tr, Te, attention="luong", dec_depth=1, kind="ordinary", seed=31):
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, mode, 0.0, decoder_depth=dec_depth, attention_type=attention,
                       honor_attention_type=True, max_batch=B, max_raw_len=max(Tr, 1), max_event_len=max(Te, 1), max_output_len=L)
    flat = rv.weights.init_weights(bc.cfg, seed=seed, gain=1.5)
    flat["b_fc"][bc.cfg.end_token] = 0.3
    if kind == "special":
        rng = np.random.default_rng(seed)
        flat["W_mem"][:] = special_weights(rng, 128)
        flat["W_att"][128:384] = special_weights(rng, 128)
    bc.set_weights_flat(flat)
    return bc


def _slab(rv, mode, Tr, Te, seed):
    raw, ev, _ = rv.synthetic.make_slab(B, max(Tr, 1), max(Te, 1), seed=seed, max_raw_pad=min(15, max(Tr - 1, 0)),
                                        max_event_pad=min(10, max(Te - 1, 0)))
    raw[PAD] = 0.0
    ev[PAD] = 0.0
    return {"joint": (raw, ev), "raw": raw, "event": ev}[mode]


def _run(bc, x, W):
    if W == "greedy":
        t, s = bc.greedy_search_prediction(x, L)
    else:
        t, s = bc.beam_search_prediction(x, W, L)
    return t.numpy().copy(), s.numpy().copy(), bc.get_tensor("chunk_steps").astype(int).copy()


def _persist_forms(bc):
    rows = bc.get_tensor("kernel_forms").reshape(-1, 5).astype(int)
    return [tuple(r[1:]) for r in rows if r[0] == K_DEC_PERSIST]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ordinary", "special"])
@pytest.mark.parametrize("mode,Tr,Te", SIZES, ids=[f"{m}-Tm{r + e}" for m, r, e in SIZES])
def test_fused_projection_is_the_gemm_bit_for_bit(rv, mode, Tr, Te, kind):
    Tm = Tr + Te
    bc = _mk(rv, mode, Tr, Te, kind=kind, seed=31 + Tm)
    x = _slab(rv, mode, Tr, Te, seed=Tm)
    bc.set_option("persist_taps", 1)
    bc.set_option("profile", 1)
    for W in (5, "greedy"):
        got = {}
        for fused in (1, 0):
            bc.set_option("fused_memory", fused)
            bc.reset_profile()
            tok, sc, cs = _run(bc, x, W)
            names = set(bc.profile())
            assert "dec_persist" in names and ("gemm_memory" in names) == (fused == 0), (W, fused, names)
            nit = 2 if Tm <= 64 else 8 if Tm <= 256 else 11
            assert _persist_forms(bc) == [(1 if W == "greedy" else W, nit, 1, 3)], (W, fused)
            got[fused] = (tok, sc, cs, bc.get_tensor("projected_memory").reshape(B, Tm, 256).copy())
        pm1, pm0 = got[1][3], got[0][3]
        bad = np.argwhere(_bits(pm1) != _bits(pm0))
        assert bad.size == 0, f"{kind} T_m={Tm} W={W}: {len(bad)} of {pm0.size} values differ, first (b, t, column) {bad[:4].tolist()}"
        if kind == "ordinary":
            assert np.isfinite(pm0).all() and np.abs(pm0[0]).max() > 1e-3       # a real product, not an untouched buffer
        assert (got[1][0] == got[0][0]).all() and _same(got[1][1], got[0][1]) and (got[1][2] == got[0][2]).all(), (kind, Tm, W)
    bc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,Tr,Te", [("raw", 17, 0), ("event", 0, 15), ("joint", 226, 30), ("joint", 227, 30)],
                         ids=["raw-Tm17", "event-Tm15", "joint-Tm256", "joint-Tm257"])
def test_default_call_without_taps_and_asynchronous_calls(rv, mode, Tr, Te):
    """No taps (what a product call runs): results identical with the option on and off; `projected_memory` of a fused call is built
    on request from that call's enc_output and is the GEMM path's tensor; asynchronous calls at depth 3 over three distinct slabs
    (one with the padding chunk) return the synchronous results of each."""
    import torch
    Tm = Tr + Te
    bc = _mk(rv, mode, Tr, Te, seed=77 + Tm)
    slabs = [_slab(rv, mode, Tr, Te, seed=200 + Tm + k) for k in range(3)]
    want = {}
    for fused in (0, 1):
        bc.set_option("fused_memory", fused)
        res = [_run(bc, x, 5) for x in slabs]
        pm = bc.get_tensor("projected_memory").reshape(B, Tm, 256).copy()      # of the last slab
        again = bc.get_tensor("projected_memory").reshape(B, Tm, 256)
        assert _same(pm, again)
        want[fused] = (res, pm)
    for (t1, s1, c1), (t0, s0, c0) in zip(want[1][0], want[0][0]):
        assert (t1 == t0).all() and _same(s1, s0) and (c1 == c0).all()
    assert _same(want[1][1], want[0][1])
    assert not any(_same(want[0][0][0][1], r[1]) for r in want[0][0][1:])        # the slabs are distinct in their scores too
    bc.set_async_depth(3)
    for fused in (1, 0):
        bc.set_option("fused_memory", fused)
        outs = list(bc.beam_search_stream(slabs + slabs, 5, L))
        assert len(outs) == 6
        for k, (t, s) in enumerate(outs):
            t0, s0, _ = want[0][0][k % 3]
            assert (t.cpu().numpy() == t0).all() and _same(s.cpu().numpy(), s0), (fused, k)
    bc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("attention,dec_depth", [("bahdanau", 1), ("luong", 2)], ids=["bahdanau", "two-cells"])
def test_other_forms_keep_the_gemm(rv, attention, dec_depth):
    """A Bahdanau handle (ATT 4) and a two-cell handle (D = 2) launch `gemm_memory` whatever the option says, and return the same
    bits either way."""
    mode, Tr, Te = "joint", 60, 12
    bc = _mk(rv, mode, Tr, Te, attention=attention, dec_depth=dec_depth, seed=5)
    x = _slab(rv, mode, Tr, Te, seed=5)
    bc.set_option("persist_taps", 1)
    bc.set_option("profile", 1)
    got = {}
    for fused in (1, 0):
        bc.set_option("fused_memory", fused)
        bc.reset_profile()
        tok, sc, cs = _run(bc, x, 5)
        names = set(bc.profile())
        assert "dec_persist" in names and "gemm_memory" in names, (fused, names)
        assert _persist_forms(bc) == [(5, 8, dec_depth, 4 if attention == "bahdanau" else 3)]
        got[fused] = (tok, sc, cs, bc.get_tensor("projected_memory").copy(), bc.get_tensor("step_logits").copy())
    for a, b in zip(got[1], got[0]):
        assert _same(a, b)
    bc.close()


# ScratchSize (bytes per lane) of the two benchmark-width instantiations of the fused form at this commit, which is also what the
# parent commit's GEMM-fed kernels compiled to: (0, 0).  tests/test_build.py allows the first 8 B; this file allows neither any.
FUSED_SCRATCH = {"k_dec_persistILi5ELi11ELi1ELi3E": 0, "k_dec_persistILi5ELi8ELi1ELi3E": 0}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_fused_forms_do_not_spill(tmp_path):
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ravvent-basecaller_amd", "csrc")
    out = tmp_path / "decode.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", os.path.join(csrc, "decode.hip"),
                    "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    found = {}
    for m in re.finditer(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(".Lfunc_end", m.start()):][:4000]
        sc, vg = re.search(r"; ScratchSize: (\d+)", tail), re.search(r"; NumVgprs: (\d+)", tail)
        if sc:
            found[m.group(1)] = (int(sc.group(1)), int(vg.group(1)))
    for pat, limit in FUSED_SCRATCH.items():
        hits = {k: v for k, v in found.items() if pat in k}
        assert len(hits) == 1, (pat, list(hits))
        for name, (scratch, vgpr) in hits.items():
            print(f"{name}: ScratchSize {scratch}, NumVgprs {vgpr}")
            assert scratch <= limit, f"{name}: {scratch} B of scratch per lane ({vgpr} VGPRs) > {limit}"
