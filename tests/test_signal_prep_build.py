"""Build-level guard of the signal preparation kernels (csrc/signal_prep.hip; CPU, hipcc cross-compiles gfx950 here), after
tests/test_windows_build.py: every kernel of the path is in the gfx950 listing and keeps its values in registers -- the peak pass's
state machine and the per-thread tile of the scan in scratch would show here and in no result."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc")
KERNELS = ["k_sp_tile_sums", "k_sp_tile_scan", "k_sp_prefix", "k_sp_tstat", "k_sp_peaks", "k_sp_events", "k_sp_fit", "k_sp_raw_scale",
           "k_sp_windows"]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("sp") / "signal_prep.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                    os.path.join(CSRC, "signal_prep.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    found = {}
    for m in re.finditer(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(".Lfunc_end", m.start()):][:4000]
        sc = re.search(r"; ScratchSize: (\d+)", tail)
        if sc:
            found[m.group(1)] = int(sc.group(1))
    return found


def test_signal_prep_kernels_exist_and_use_no_scratch(listing):
    for w in KERNELS:
        hits = {k: v for k, v in listing.items() if re.search(r"\d+" + w + "E", k)}
        assert len(hits) == 1, (w, sorted(listing))
        (name, scratch), = hits.items()
        print(f"{name}: ScratchSize {scratch}")
        assert scratch == 0, f"{name}: {scratch} B of scratch per lane"


def test_makefile_builds_it_without_contraction():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("signal_prep.o:"):]
    assert "-ffp-contract=off" in rule[:rule.index("\n\n")], "sumsq / len - m * m must not become an fma"
    assert "signal_prep.hip" in mk[mk.index("SRCS ="):mk.index("OBJS =")]
