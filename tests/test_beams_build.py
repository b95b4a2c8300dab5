"""Build-level guard of the all-beams finalize kernel (CPU, hipcc cross-compiles gfx950 here), after tests/test_build.py: the kernel
keeps the chunk's records, the back-traced tokens and the slots in LDS and walks them with run-time loops; a change that turns one of
them into a per-lane array would put it in scratch, and no result would say so."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_finalize_beams_uses_no_scratch(tmp_path):
    out = tmp_path / "beams.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    os.path.join(CSRC, "beams.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    found = {}
    for m in re.finditer(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(".Lfunc_end", m.start()):][:4000]
        sc = re.search(r"; ScratchSize: (\d+)", tail)
        lds = re.search(r"; LDSByteSize: (\d+)", tail)
        if sc:
            found[m.group(1)] = (int(sc.group(1)), int(lds.group(1)) if lds else -1)
    hits = {k: v for k, v in found.items() if "k_dec_finalize_beams" in k}
    assert len(hits) == 1, sorted(found)
    (name, (scratch, lds)), = hits.items()
    print(f"{name}: ScratchSize {scratch}, LDS {lds} B")
    assert scratch == 0, f"{name}: {scratch} B of scratch per lane"
    assert 0 < lds <= 16 * 1024, f"{name}: {lds} B of LDS (five [64 x 8] tables of 4 bytes = 10 KB)"
