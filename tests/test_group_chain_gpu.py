"""The chain of a coalesced group: members' device inputs read where they are (option `group_inplace`) and the event encoder on a side
stream beside the raw one (option `group_side_ev`).  Both only move where bytes are read from and on which stream an independent chain
runs, so every member of every group must get the tokens, the score bits and the S of its own synchronous call.

Shapes: the smallest that exercise the member arithmetic of the layer-0 kernels -- joint mode, T = 24 + 6, L = 6, beam 5 and beam 1,
base-emitting weights, slabs of 15, 1, 17, 16 and 40 chunks so that the 16-chunk recurrence workgroups straddle member boundaries and
the last workgroup of every group reaches beyond it.  Device inputs are views at odd float offsets into one device tensor: 4-byte
alignment only.  Groups run on their own contexts, whose mask cannot be tapped (rv_get_tensor answers from the handle's context), so
the all-padding case compares the tokens and scores of both neighbours."""
import warnings

import numpy as np
import pytest

from test_coalesce_gpu import _same, _stats
from test_parity_gpu import _emitting_flat

pytestmark = pytest.mark.gpu

T_R, T_E, L = 24, 6, 6
BEAMS = (5, 1)
SIZES = (15, 1, 17, 16, 40, 15, 17)      # slab 5: its last chunk is all padding in its raw part; slab 6: a second 17 for the lifetime case
PAD_SLAB, SECOND_17 = 5, 6
# members (slab indices) of the groups: chunks 57, 57, 89 and 32 + the padding pair -- boundaries at 17 | 1, 17 | 15, 16, 33, 49 | 15
GROUPS = ((2, 4), (1, 3, 4), (0, 1, 2, 3, 4), (PAD_SLAB, 2))
OPTIONS = ((-1, 1), (0, 0), (0, 1), (1, 0), (1, 1))      # (group_side_ev, group_inplace): the defaults, then the four combinations


def _odd_views(torch, arrays):
    """Every array as a view at an odd float offset into ONE device tensor."""
    total = 1 + sum(a.size + (a.size & 1) for a in arrays)
    pool = torch.zeros(total, dtype=torch.float32, device="cuda")
    off, views = 1, []
    for a in arrays:
        v = pool[off:off + a.size].view(*a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.is_contiguous() and v.data_ptr() % 8 == 4
        views.append(v)
        off += a.size + (a.size & 1)
    return pool, views


@pytest.fixture(scope="module")
def world(rv):
    """One handle, the slabs (host arrays and odd-offset device views) and their synchronous results per beam width, computed once."""
    import torch
    bc = rv.Basecaller(128, 128, 128, rv.data_loader.nuc_tk, "joint", 0.0, encoder_depth=2, attention_type="luong",
                       honor_attention_type=True, max_batch=40, max_raw_len=T_R, max_event_len=T_E, max_output_len=L)
    bc.set_weights_flat(_emitting_flat(rv, bc.cfg))
    slabs = [rv.synthetic.make_slab(n, T_R, T_E, seed=300 + i, max_raw_pad=8, max_event_pad=3)[:2] for i, n in enumerate(SIZES)]
    slabs[PAD_SLAB][0][-1] = 0.0
    assert not slabs[PAD_SLAB][0][-1].any() and slabs[PAD_SLAB][1][-1, 0].all() and slabs[2][0][0, :T_R - 8].all()
    pool, views = _odd_views(torch, [a for s in slabs for a in s])
    dev = [(views[2 * i], views[2 * i + 1]) for i in range(len(slabs))]
    ref = {}
    for W in BEAMS:
        for i, x in enumerate(dev):
            t, s = bc.beam_search_prediction(x, W, L)
            t, s = t.cpu().numpy().copy(), s.cpu().numpy().copy()
            t.setflags(write=False); s.setflags(write=False)
            ref[W, i] = (t, s, int(t.shape[1]))
    assert all(r[2] > 0 for r in ref.values())
    assert any(not np.array_equal(ref[5, 2][0][:1], ref[5, i][0][:1]) for i in (3, 4, 6)), "every member has its own data"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # (more contexts than hardware queues: what coalescing is for)
        bc.set_async_depth(10)
    yield {"bc": bc, "slabs": slabs, "dev": dev, "ref": ref, "pool": pool}
    bc.close()


def _options(bc, side_ev, inplace):
    bc.set_option("group_side_ev", side_ev)
    bc.set_option("group_inplace", inplace)


def _run_group(bc, inputs, members, W):
    """Submit the members as one group -> their results, and what coalesce_stats says was launched meanwhile."""
    bc.set_coalesce(len(members))
    g0, s0, _, in_force = _stats(bc)
    assert in_force == len(members)
    tickets = [bc.submit_beam_search(inputs[i], W, L) for i in members]
    g1, s1, largest, _ = _stats(bc)
    assert (g1 - g0, s1 - s0) == (1, len(members)) and largest >= len(members), (g0, s0, g1, s1, largest)
    return [bc.collect(t) for t in tickets]


@pytest.mark.parametrize("W", BEAMS)
@pytest.mark.parametrize("side_ev,inplace", OPTIONS)
def test_members_straddling_workgroups_equal_synchronous(world, side_ev, inplace, W):
    """Groups of 2, 3 and 5 members and the padding pair, device inputs at 4-byte alignment, under the default options and each of the
    four combinations: per member tokens, score bits and S of the synchronous call; the groups were really formed."""
    bc, dev, ref = world["bc"], world["dev"], world["ref"]
    _options(bc, side_ev, inplace)
    try:
        for members in GROUPS:
            assert any(sum(SIZES[i] for i in members[:k]) % 16 for k in range(1, len(members))), "a workgroup straddles two members"
            assert members == GROUPS[-1] or sum(SIZES[i] for i in members) % 16, "the last workgroup reaches beyond the group"
            got = _run_group(bc, dev, members, W)
            for i, g in zip(members, got):
                assert _same(g, ref[W, i]), (members, i)
    finally:
        _options(bc, -1, 1)


def test_all_padding_tail_beside_an_ordinary_chunk(world):
    """A member whose last chunk is all padding in its raw part, in the same workgroup as its neighbour's ordinary first chunk: both
    members equal their synchronous calls, and the padding chunk's row is not its neighbour's."""
    bc, dev, ref = world["bc"], world["dev"], world["ref"]
    got = _run_group(bc, dev, (PAD_SLAB, 2), 5)
    assert _same(got[0], ref[5, PAD_SLAB]) and _same(got[1], ref[5, 2])
    got = _run_group(bc, dev, (0, 2), 5)        # the same neighbour behind the slab of the same size without the padding chunk
    assert _same(got[0], ref[5, 0]) and _same(got[1], ref[5, 2])


def test_group_launched_before_it_is_full(world):
    """Fewer members than the group's capacity: launched by the collect of a ticket, and by a synchronous call in between."""
    bc, dev, ref = world["bc"], world["dev"], world["ref"]
    bc.set_coalesce(3)
    g0 = _stats(bc)[0]
    t = [bc.submit_beam_search(dev[i], 5, L) for i in (2, 4)]
    assert _stats(bc)[0] == g0
    assert _same(bc.collect(t[1]), ref[5, 4]) and _stats(bc)[0] == g0 + 1
    assert _same(bc.collect(t[0]), ref[5, 2])
    t = [bc.submit_beam_search(dev[i], 5, L) for i in (0, 3)]
    mid = bc.beam_search_prediction(dev[1], 5, L)
    assert _stats(bc)[0] == g0 + 2 and _same(mid, ref[5, 1])
    assert _same(bc.collect(t[0]), ref[5, 0]) and _same(bc.collect(t[1]), ref[5, 3])


@pytest.mark.parametrize("side_ev", [0, 1])
def test_host_input_group_is_unchanged(world, side_ev):
    bc, slabs, ref = world["bc"], world["slabs"], world["ref"]
    _options(bc, side_ev, 1)
    try:
        got = _run_group(bc, slabs, (0, 1, 2, 3, 4), 5)
        assert all(_same(g, ref[5, i]) for i, g in enumerate(got))
    finally:
        _options(bc, -1, 1)


def test_input_storage_reused_after_collect(world):
    """Device inputs are the caller's again once the ticket is collected: overwritten then and submitted from the same storage, the
    second group decodes the new data."""
    import torch
    bc, dev, slabs, ref = world["bc"], world["dev"], world["slabs"], world["ref"]
    assert not _same((ref[5, SECOND_17][0], ref[5, SECOND_17][1]), ref[5, 2]), "the two slabs of 17 decode differently"
    pool, (raw, ev) = _odd_views(torch, list(slabs[2]))
    inputs = {2: (raw, ev), 4: dev[4]}
    got = _run_group(bc, inputs, (2, 4), 5)
    assert _same(got[0], ref[5, 2]) and _same(got[1], ref[5, 4])
    raw.copy_(torch.from_numpy(slabs[SECOND_17][0])); ev.copy_(torch.from_numpy(slabs[SECOND_17][1]))
    got = _run_group(bc, inputs, (2, 4), 5)
    assert _same(got[0], ref[5, SECOND_17]) and _same(got[1], ref[5, 4])


def test_option_values_are_validated(world, rv):
    bc = world["bc"]
    for key, bad in (("group_inplace", 2), ("group_inplace", -1), ("group_side_ev", 2), ("group_side_ev", -2)):
        with pytest.raises(rv._capi.RavventHipError, match=key):
            bc.set_option(key, bad)
    got = _run_group(bc, world["dev"], (2, 4), 5)      # the refused values changed nothing
    assert _same(got[0], world["ref"][5, 2]) and _same(got[1], world["ref"][5, 4])
