"""Build-level guard of the window kernels of lstm_mx.hip (CPU; hipcc cross-compiles gfx950 here), after tests/test_build.py: the
window kind of the matrix-pipe layer-0 recurrence (F = 1 and 5, CH = 16 and 8) keeps its staging values in registers -- a per-lane
array in scratch would show here and in no result -- and so does k_expand_windows.  The chunk-tensor and member instantiations must
still be there beside them, untouched by name."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("mx") / "lstm_mx.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    os.path.join(CSRC, "lstm_mx.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    found = {}
    for m in re.finditer(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(".Lfunc_end", m.start()):][:4000]
        sc = re.search(r"; ScratchSize: (\d+)", tail)
        if sc:
            found[m.group(1)] = int(sc.group(1))
    return found


def test_window_kernels_use_no_scratch(listing):
    want = [f"k_lstm_rec_mx_windowsILi{F}ELi{CH}EEE" for F in (1, 5) for CH in (16, 8)] + ["k_expand_windows"]
    for w in want:
        hits = {k: v for k, v in listing.items() if w in k}
        assert len(hits) == 1, (w, sorted(listing))
        (name, scratch), = hits.items()
        print(f"{name}: ScratchSize {scratch}")
        assert scratch == 0, f"{name}: {scratch} B of scratch per lane"


def test_existing_instantiations_are_still_built(listing):
    for F in (0, 1, 5):
        for CH in (16, 8):
            assert any(f"13k_lstm_rec_mxILi{F}ELi{CH}EEE" in k for k in listing), (F, CH)
            if F:
                assert any(f"k_lstm_rec_mx_membersILi{F}ELi{CH}EEE" in k for k in listing), (F, CH)
    assert len([k for k in listing if "k_lstm_rec_mx_windows" in k]) == 4, "no window form of the pre-projected layers (F = 0)"
