"""Build-level guard of the moves finalize kernel (CPU, hipcc cross-compiles gfx950 here), after tests/test_beams_build.py: the
kernel keeps the chunk's parents and the rows of the back-trace in LDS and walks them with run-time loops, and reads the records from
global memory where it uses them; a per-lane array or an LDS table of the records would show here and in no result."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_finalize_moves_uses_no_scratch(tmp_path):
    out = tmp_path / "moves.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    os.path.join(CSRC, "moves.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    found = {}
    for m in re.finditer(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(".Lfunc_end", m.start()):][:4000]
        sc = re.search(r"; ScratchSize: (\d+)", tail)
        lds = re.search(r"; LDSByteSize: (\d+)", tail)
        if sc:
            found[m.group(1)] = (int(sc.group(1)), int(lds.group(1)) if lds else -1)
    hits = {k: v for k, v in found.items() if "k_dec_finalize_moves" in k}
    assert len(hits) == 1, sorted(found)
    (name, (scratch, lds)), = hits.items()
    print(f"{name}: ScratchSize {scratch}, LDS {lds} B")
    assert scratch == 0, f"{name}: {scratch} B of scratch per lane"
    # two [64 steps x 8 beams] tables of 4 bytes (parents, rows) = 4 KB, and the slab's S: a third table would pass 6 KB
    assert 0 < lds <= 4 * 1024 + 64, f"{name}: {lds} B of LDS (two [64 x 8] tables of 4 bytes = 4 KB)"
