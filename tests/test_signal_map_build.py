"""Build-level guard of the two signal-map kernels of moves.hip (CPU; hipcc cross-compiles gfx950 here), after
tests/test_gru_build.py: k_dec_finalize_calls_moves and k_forced_moves are there beside k_dec_finalize_moves, and none of the three
keeps anything in scratch -- their working set is a handful of registers and, for the compaction, 1.5 KB of LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc")


@pytest.fixture(scope="module")
def moves(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("signal_map") / "moves.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    os.path.join(CSRC, "moves.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    found = {}
    for m in re.finditer(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(".Lfunc_end", m.start()):][:4000]
        sc, vg, lds = re.search(r"; ScratchSize: (\d+)", tail), re.search(r"; NumVgprs: (\d+)", tail), re.search(r"; LDSByteSize: (\d+)", tail)
        if sc and vg:
            found[m.group(1)] = (int(sc.group(1)), int(vg.group(1)), int(lds.group(1)) if lds else -1)
    return found


def test_signal_map_kernels_are_built_without_scratch(moves):
    for w in ("26k_dec_finalize_calls_moves", "14k_forced_moves", "20k_dec_finalize_moves"):
        hits = {k: v for k, v in moves.items() if w in k}
        assert len(hits) == 1, (w, sorted(moves))
        (name, (scratch, vgprs, lds)), = hits.items()
        print(f"{name}: ScratchSize {scratch}, NumVgprs {vgprs}, LDS {lds} B")
        assert scratch == 0, f"{name}: {scratch} B of scratch per lane"
        assert vgprs <= 128, (name, vgprs)
    assert len(moves) == 3, sorted(moves)
