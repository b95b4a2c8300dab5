"""Build-level guard of the persistent GRU decode (CPU, hipcc cross-compiles gfx950 here), from the device listing of csrc/decode.hip:
every form of the GRU list -- k_dec_persist_gru<W, NIT, ATT>, restated here -- is emitted exactly once, and none spills more than the
BiLSTM form it shares its body with, k_dec_persist<W, NIT, 1, ATT> of the same listing: the GRU gate phase holds one state vector and
five transcendentals per unit against the LSTM's two and six, so it has no reason to need a register more.  The yardstick is the
existing kernel, not a constant."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc")

# the GRU list (decode.hip, for_each_persist_form_gru): every beam width, the three NIT bands, Luong (3) and Bahdanau (4)
GRU_FORMS = [(W, NIT, ATT) for W in range(1, 9) for ATT in (3, 4) for NIT in (2, 8, 11)]


def scratch_by_kernel(text):
    """{mangled kernel symbol: [ScratchSize, ...]} of a -S --cuda-device-only listing (one entry per emission)."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):", text, re.M):
        end = text.find(".Lfunc_end", m.start())
        if end < 0:
            continue
        sc = re.search(r"; ScratchSize: (\d+)", text[end:end + 4000])
        if sc:
            out.setdefault(m.group(1), []).append(int(sc.group(1)))
    return out


def check_listing(text):
    found = scratch_by_kernel(text)
    gru = {k: v for k, v in found.items() if "k_dec_persist_gruI" in k}
    seen = {}
    for name, sizes in gru.items():
        m = re.search(r"k_dec_persist_gruILi(\d+)ELi(\d+)ELi(\d+)EE", name)
        assert m, name
        seen.setdefault(tuple(int(g) for g in m.groups()), []).extend(sizes)
    assert sorted(seen) == sorted(GRU_FORMS), (sorted(set(GRU_FORMS) - set(seen)), sorted(set(seen) - set(GRU_FORMS)))
    assert all(len(v) == 1 for v in seen.values()), {k: len(v) for k, v in seen.items() if len(v) != 1}
    worse = {}
    for (W, NIT, ATT), (scratch,) in sorted(seen.items()):
        twin = [v for k, v in found.items() if re.search(r"k_dec_persistILi%dELi%dELi1ELi%dEE" % (W, NIT, ATT), k)]
        assert len(twin) == 1 and len(twin[0]) == 1, (W, NIT, ATT, "the BiLSTM form of the same shape is the yardstick", twin)
        print(f"k_dec_persist_gru<{W},{NIT},{ATT}>: {scratch} B of scratch per lane, k_dec_persist<{W},{NIT},1,{ATT}>: {twin[0][0]}")
        if scratch > twin[0][0]:
            worse[(W, NIT, ATT)] = (scratch, twin[0][0])
    assert not worse, f"GRU forms that spill more than their BiLSTM counterparts (gru, lstm): {worse}"


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_every_gru_form_is_emitted_once_and_spills_no_more_than_its_lstm_form(tmp_path):
    out = tmp_path / "decode.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", os.path.join(CSRC, "decode.hip"),
                    "-o", str(out)], check=True, capture_output=True)
    check_listing(out.read_text())
