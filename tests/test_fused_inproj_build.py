"""k_lstm_rec_mx_proj (option fused_inproj) as it compiles for gfx950: no scratch, at most 256 VGPRs (two waves per SIMD), its dynamic LDS
inside a CU's 160 KB at every T (it does not depend on T); and the kernels lstm_mx.hip held before it -- the six forms of k_lstm_rec_mx,
their _members and _windows variants, k_inproj_small, k_expand_windows -- keep the instruction streams and resources they had at the
commit before the projecting form (tests/golden/lstm_mx_forms_isa.json: tools/isa_diff.py's digest of each kernel's body, recorded from
that commit; `tools/isa_diff.py --max-move 1` of the two listings reports them identical).

The digests pin the compiler's output as well as the source: they are meant to be RE-RECORDED whenever those kernels are changed on purpose
or the toolchain moves, after `tools/isa_diff.py` of the old and new listings has been read.  To re-record, from the repository root:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only ravvent-basecaller_amd/csrc/lstm_mx.hip -o lstm_mx.s
    python tests/test_fused_inproj_build.py lstm_mx.s        # rewrites tests/golden/lstm_mx_forms_isa.json (all kernels but the projecting form)"""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ravvent-basecaller_amd", "csrc")
PROJ = "k_lstm_rec_mx_proj"
# MXP_LDS of lstm_mx.hip: the h image, three [512] float tables, two fragment buffers of two timesteps x two parts x 8 KB
PROJ_LDS = 16384 + 3 * 512 * 4 + 2 * (2 * 2 * 8192)


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("mx") / "lstm_mx.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", os.path.join(CSRC, "lstm_mx.hip"),
                    "-o", str(out)], check=True, capture_output=True)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_diff
    finally:
        sys.path.pop(0)
    return isa_diff.kernels(str(out))


def test_projecting_form_resources(listing):
    hits = {k: v for k, v in listing.items() if PROJ in k}
    assert len(hits) == 1, list(hits)
    (name, (_, count, meta)), = hits.items()
    print(f"{name}: {count} instructions, {meta}")
    assert meta["ScratchSize"] == 0, meta
    assert meta["NumVgprs"] <= 256, meta
    assert meta["LDSByteSize"] + PROJ_LDS <= 160 * 1024, (meta, PROJ_LDS)
    src = open(os.path.join(CSRC, "lstm_mx.hip")).read()
    assert "constexpr int MXP_NT = 2;" in src and "constexpr int MXP_LDS = 16384 + 3 * RV_G * (int)sizeof(float) + 2 * MXP_FRAG;" in src, \
        "PROJ_LDS above restates these constants"


def test_existing_forms_did_not_move(listing):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "lstm_mx_forms_isa.json")))
    assert len(gold) >= 17
    for name, g in gold.items():
        assert name in listing, f"{name} is gone"
        digest, count, meta = listing[name]
        assert count == g["instructions"] and meta == g["meta"], (name, count, meta, g)
        assert digest == g["hash"], f"{name}: the instruction stream moved"
    assert sorted(set(listing) - set(gold)) == [k for k in sorted(listing) if PROJ in k]


if __name__ == "__main__":      # re-record the digests from a listing (see the head of this file)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_diff
    rec = {name: {"hash": v[0], "instructions": v[1], "meta": v[2]} for name, v in sorted(isa_diff.kernels(sys.argv[1]).items()) if PROJ not in name}
    json.dump(rec, open(os.path.join(ROOT, "tests", "golden", "lstm_mx_forms_isa.json"), "w"), indent=1, sort_keys=True)
    print(f"{len(rec)} kernels recorded")
