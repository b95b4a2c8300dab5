"""The inputs of tests/test_longest_output_gpu.py meet their conditions, on the oracle alone: the numpy fp32 twin follows the fp64
decode on every chunk for all 63 steps with scores within 4e-5, and the fp64 records exercise what the L-sized kernels can get wrong
(longest_output_inputs.assert_long / assert_spread / assert_ragged; the GPU module's docstring says why each matters)."""
import numpy as np
import pytest

import longest_output_inputs as I
from test_beams_gpu import _assert_not_vacuous


@pytest.mark.parametrize("fam,name,W,shape,split", I.ALL, ids=lambda v: str(v))
def test_inputs_meet_their_conditions(rv, oracle, fam, name, W, shape, split):
    tag = f"{fam} {name} W={W} shape {shape}" + (" B=70" if split else "")
    p = I.passes(rv, oracle, fam, name, W, shape, split)
    e = p["e"]
    print(f"{tag}: finished at {e['fin_at'].tolist()}, twin {p['twin']}, largest |score| "
          f"{np.abs(p['o']['sc'][np.isfinite(p['o']['sc'])]).max():.1f}")
    I.assert_twin_follows(p, tag)
    _assert_not_vacuous(e, W, tag, finish_apart=name != "long")
    if name == "long":
        I.assert_long(e, W, tag)
    else:
        I.assert_spread(e, W, tag)
    if name != "long":                       # hypothesis 0 of some chunk ends at its first step: the one-token case of the short end
        assert W == 1 or (e["lengths"][:, 0] == 1).any(), (tag, "no hypothesis 0 of length 1", e["lengths"][:, 0].tolist())


@pytest.mark.parametrize("fam", ["luong1", "bahdanau1"])
def test_ragged_best_call(rv, oracle, fam):
    p = I.passes(rv, oracle, fam, "ragged", 1)
    counts, inner = I.assert_ragged(p["o"]["tokens"][:, :, 0], fam)
    print(f"{fam}: best-hypothesis lengths {p['e']['lengths'][:, 0].tolist()}, letters {counts.tolist()}, rows with an inner non-letter {inner}")
    if fam == "luong1":                      # the rows the fused post-processing is shown: a 63-letter row and a compacted one
        assert counts[inner].max() >= 40, (fam, "the compacted row is short", counts.tolist(), inner)


def test_greedy_inputs(rv, oracle):
    g = I.greedy_passes(rv, oracle)
    assert g["og"].shape == (6, I.STEPS) and np.array_equal(g["tg"], g["og"]), "the twin's greedy ids leave the fp64 decode"
    err = float(np.abs(g["tlg"] - g["olg"]).max())
    assert err <= I.TWIN_SCORE_BOUND, err
    early = I.greedy_passes(rv, oracle, rows=I.GREEDY_EARLY_ROWS)
    S = early["og"].shape[1]
    assert 2 <= S < HALF_ and np.array_equal(early["tg"], early["og"]), ("the three rows must stop early", S)


HALF_ = I.HALF
