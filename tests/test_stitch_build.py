"""Build-level guard of the stitch kernels (csrc/stitch.hip; CPU, hipcc cross-compiles gfx950 here), after
tests/test_signal_prep_build.py: the three stages -- positions and keep ranges, the exclusive scan (three launches, signal_prep.hip's
pattern), the scatter -- are each in the gfx950 listing once and keep their values in registers, the file uses no atomics, and the
Makefile builds it without floating-point contraction: c_i + (e - i) (c_j - c_i) as an fma would not be signal_positions' bits."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc")
KERNELS = ["k_st_keep", "k_st_scan_tiles", "k_st_scan_carry", "k_st_scan_offsets", "k_st_scatter"]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("st") / "stitch.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                    os.path.join(CSRC, "stitch.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    found = {}
    for m in re.finditer(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(".Lfunc_end", m.start()):][:4000]
        sc = re.search(r"; ScratchSize: (\d+)", tail)
        if sc:
            found[m.group(1)] = int(sc.group(1))
    return found, text


def test_stitch_kernels_exist_once_and_use_no_scratch(listing):
    found, _ = listing
    for w in KERNELS:
        hits = {k: v for k, v in found.items() if re.search(r"\d+" + w + "E", k)}
        assert len(hits) == 1, (w, sorted(found))
        (name, scratch), = hits.items()
        print(f"{name}: ScratchSize {scratch}")
        assert scratch == 0, f"{name}: {scratch} B of scratch per lane"
    assert len(found) == len(KERNELS), sorted(found)


def test_no_atomics_and_no_fma(listing):
    _, text = listing
    assert not re.search(r"\b\w*atomic\w*\b", text.split(".amdgpu_metadata")[0], re.I), "the stitch uses no atomics"
    assert not re.search(r"\bv_fma_f64\b|\bv_fmac_f64\b", text), "a contracted fp64 product-sum: not signal_positions' arithmetic"
    src = open(os.path.join(CSRC, "stitch.hip")).read()
    assert "atomic" not in re.sub(r"//.*", "", src)


def test_makefile_builds_it_without_contraction():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("stitch.o:"):]
    assert "-ffp-contract=off" in rule[:rule.index("\n\n")], "c_i + (e - i) * (c_j - c_i) must not become an fma"
    assert "stitch.hip" in mk[mk.index("SRCS ="):mk.index("OBJS =")]
