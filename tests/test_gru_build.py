"""Build-level guard of the BiGRU kernels of gru_mx.hip (CPU; hipcc cross-compiles gfx950 here), after tests/test_windows_build.py:
every k_gru_rec_mx form and k_dec_cell_gru is there and keeps its state in registers -- 96 VGPRs of resident recurrent fragments beside
the step's working set: a spill would show here and in no result -- and lstm_mx.hip still yields its instantiations beside them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc")


def _listing(tmp_path_factory, src):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("gru") / (src + ".s")
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    os.path.join(CSRC, src), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    found = {}
    for m in re.finditer(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(".Lfunc_end", m.start()):][:4000]
        sc, vg = re.search(r"; ScratchSize: (\d+)", tail), re.search(r"; NumVgprs: (\d+)", tail)
        if sc and vg:
            found[m.group(1)] = (int(sc.group(1)), int(vg.group(1)))
    return found


@pytest.fixture(scope="module")
def gru(tmp_path_factory):
    return _listing(tmp_path_factory, "gru_mx.hip")


@pytest.fixture(scope="module")
def lstm(tmp_path_factory):
    return _listing(tmp_path_factory, "lstm_mx.hip")


def test_gru_kernels_are_built_without_scratch(gru):
    want = [f"12k_gru_rec_mxILi{F}ELi16EEE" for F in (0, 1, 5)] + ["14k_dec_cell_gru"]
    for w in want:
        hits = {k: v for k, v in gru.items() if w in k}
        assert len(hits) == 1, (w, sorted(gru))
        (name, (scratch, vgprs)), = hits.items()
        print(f"{name}: ScratchSize {scratch}, NumVgprs {vgprs}")
        assert scratch == 0, f"{name}: {scratch} B of scratch per lane"
        assert vgprs <= 256, (name, vgprs)                # 512 threads: two waves per SIMD
    assert len([k for k in gru if "k_gru_rec_mx" in k]) == 3, "sixteen chunks per workgroup only; no members or windows source"


def test_lstm_mx_instantiations_are_still_built(lstm):
    for F in (0, 1, 5):
        for CH in (16, 8):
            assert any(f"13k_lstm_rec_mxILi{F}ELi{CH}EEE" in k for k in lstm), (F, CH)
    assert not any("gru" in k for k in lstm)
