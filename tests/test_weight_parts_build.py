"""The one-part forms of the persistent decode (csrc/decode.hip: k_dec_persist_1p, option weight_parts 1) as they compile for gfx950:
every form of the one-part list exists under its own kernel name, the two benchmark-width forms keep the resident rows in registers
as their two-part counterparts must (tests/test_build.py), and the two-part kernels are still there under their names.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ravvent-basecaller_amd", "csrc")

ONE_PART = [(W, NIT) for W in (1, 5) for NIT in (2, 8, 11)]     # k_dec_persist_1p<W, NIT, 3>: for_each_persist_form_1p
# max bytes of scratch per lane of every one-part form: the bound tests/test_build.py sets for the two-part counterpart where it sets
# one -- k_dec_persist<5, 11, 1, 3> (C3) 8 B, <5, 8, 1, 3> (R) 0 B -- and 0 B, what each compiles to, for the others
LIMITS = {(W, NIT): 0 for W, NIT in ONE_PART}
LIMITS[(5, 11)] = 8
TWO_PART = [r"k_dec_persistILi5ELi11ELi1ELi3E", r"k_dec_persistILi5ELi8ELi1ELi3E", r"k_dec_persistILi1ELi2ELi1ELi3E",
            r"k_dec_persistILi8ELi11ELi1ELi3E", r"k_dec_persistILi5ELi11ELi1ELi4E", r"k_dec_persistILi5ELi11ELi2ELi3E",
            r"k_dec_persistILi5ELi11ELi1ELi0E"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_one_part_forms_exist_and_do_not_spill(tmp_path):
    out = tmp_path / "decode.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", os.path.join(CSRC, "decode.hip"),
                    "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    found = {}
    for m in re.finditer(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(".Lfunc_end", m.start()):][:4000]
        sc, vg = re.search(r"; ScratchSize: (\d+)", tail), re.search(r"; NumVgprs: (\d+)", tail)
        if sc:
            found[m.group(1)] = (int(sc.group(1)), int(vg.group(1)))
    for W, NIT in ONE_PART:
        hits = {k: v for k, v in found.items() if f"k_dec_persist_1pILi{W}ELi{NIT}ELi3E" in k}
        assert len(hits) == 1, f"k_dec_persist_1p<{W}, {NIT}, 3>: {sorted(hits)}"
        (name, (scratch, vgpr)), = hits.items()
        print(f"{name}: {scratch} B of scratch per lane, {vgpr} VGPRs")
        assert scratch <= LIMITS[(W, NIT)], f"{name}: {scratch} B of scratch per lane ({vgpr} VGPRs) > {LIMITS[(W, NIT)]}"
    assert sum("k_dec_persist_1p" in k for k in found) == len(ONE_PART), "a one-part form that the list of this test does not hold"
    for pat in TWO_PART:
        assert any(re.search(pat, k) for k in found), f"no kernel matches {pat}"
