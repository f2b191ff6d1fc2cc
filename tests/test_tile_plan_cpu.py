"""CPU: the graph families of tests/tile_plan_ref.py reach the tile caps they are meant to reach (conditions on the INPUTS of
tests/test_gpu_tile_caps.py, asserted on the planner restatement - a generator that drifts cannot quietly stop reaching a
cap), and the restatement reproduces the tile counts of the committed SMPL-like fixture."""
import numpy as np
import pytest

import helpers
import tile_plan_ref as tp


def _tiles(p, k):
    return np.array(p.plan[k])          # columns: first row, rows, union, entries, padded


@pytest.mark.parametrize("name", ["cliques56", "cliques56p"])
def test_cliques56_every_tile_sits_on_the_entry_cap(name):
    L, p = tp.family(name)
    assert (p.n_real, p.n_fake, p.max_row) == (560, 400, 56)
    for k in (0, 1):
        a = _tiles(p, k)
        assert (a[:, 1] == 16).all() and (a[:, 3] == tp.ECAP).all() and (a[:, 4] == tp.ECAP).all()
    a = _tiles(p, 2)
    if name == "cliques56":
        assert (a[:-1, 3] == tp.ECAP).all() and a[-1, 3] == 448           # 280 paired rows: 17 tiles of 16 and one of 8
    else:                                # paired rows of a renumbered graph join two cliques: 264 tiny tiles
        assert len(a) == 264 and a[:, 1].min() == 1 and a[:, 1].max() == 4 and (a[:, 1] == 1).sum() == 160
        assert p.row_len[2].max() == 112


def test_cliques28_tiles_full_in_rows_and_entries_at_once():
    L, p = tp.family("cliques28")
    for k in (0, 1, 2):
        a = _tiles(p, k)
        assert ((a[:, 1] == tp.RMAX) & (a[:, 3] == tp.ECAP)).any()
        assert a[:, 3].max() == tp.ECAP


def test_cliques29_row_lengths_one_mod_four_fill_the_padded_table():
    L, p = tp.family("cliques29")
    assert (p.row_len[0] == 29).all()
    for k in (0, 1):
        a = _tiles(p, k)
        assert a[:, 1].max() == 30 and a[:, 3].max() == 870 and a[:, 4].max() == 960
    assert _tiles(p, 2)[:, 4].max() == 956


@pytest.mark.parametrize("name", ["cliques120", "cliques120p"])
def test_cliques120_every_tile_at_the_union_cap(name):
    L, p = tp.family(name)
    a = _tiles(p, 0)
    assert (a[:, 2] == tp.UCAP).all() and (p.row_len[0] == 120).all()
    assert (a[:, 1] == 1).sum() == 10 and a[:, 1].max() == 7
    assert p.plan[1] is not None
    if name == "cliques120":
        assert p.plan[2] is not None and _tiles(p, 2)[:, 2].max() == tp.UCAP
    else:
        assert p.plan[2] is None and p.n_pair_real == 0


def test_cliques121_only_the_unpooled_plan_exists():
    L, p = tp.family("cliques121")
    assert p.max_row == 121
    assert p.plan[0] is None and p.plan[1] is not None and p.plan[2] is None
    assert p.row_len[1].max() == 121 and _tiles(p, 1)[:, 2].max() == 61           # two entries per union column


@pytest.mark.parametrize("name", ["hub120", "hub120p"])
def test_hub120_the_hub_is_a_one_row_tile_at_the_union_cap(name):
    L, p = tp.family(name)
    assert p.max_row == 120
    a = _tiles(p, 0)
    one = a[a[:, 1] == 1]
    assert len(one) == 1 and one[0, 2] == tp.UCAP and one[0, 3] == 120 and p.row_len[0][one[0, 0]] == 120
    assert p.row_len[0].min() == 25 and p.row_len[0].max() == 120
    assert p.plan[1] is not None and p.plan[2] is None


@pytest.mark.parametrize("name", ["hub121", "hub121p"])
def test_hub121_one_row_over_the_cap_leaves_only_the_unpooled_plan(name):
    L, p = tp.family(name)
    assert p.max_row == 121
    assert p.plan[0] is None and p.plan[2] is None
    a = _tiles(p, 1)
    hub_row = int(np.argmax(p.row_len[1]))
    first, rows = a[(a[:, 0] <= hub_row) & (hub_row < a[:, 0] + a[:, 1])][0, :2]
    lens = sorted(p.row_len[1][first:first + rows].tolist())
    # renumbered: the hub alone in its tile; in the generator's own numbering it shares a tile with ONE band row (121 and 25
    # entries side by side, the most uneven pair a producer wave can get) and the pendant vertex is the one-row tile
    assert lens == ([121] if name == "hub121p" else [25, 121])
    assert (a[:, 1] == 1).sum() >= 1


@pytest.mark.parametrize("name", ["mixed", "mixedp"])
def test_mixed_tiles_hold_rows_of_very_different_lengths(name):
    L, p = tp.family(name)
    assert p.max_row >= 100 and p.plan[0] is not None and p.plan[1] is not None
    a = _tiles(p, 0)
    spread = [p.row_len[0][f:f + r].max() / p.row_len[0][f:f + r].min() for f, r in a[:, :2]]
    assert max(spread) >= 4.0
    assert (a[:, 1] == 1).sum() >= 1
    assert a[:, 2].max() == tp.UCAP
    if name == "mixedp":
        assert a[:, 3].max() == 881 and a[:, 4].max() == 924 and (a[:, 1] == 1).sum() == 16 and a[:, 1].max() == 28


def test_every_family_respects_the_caps_and_covers_its_rows():
    for name in tp.FAMILIES:
        L, p = tp.family(name)
        assert np.array_equal(np.sort(p.real_order), np.where(~p.fake)[0])
        for k in range(3):
            if p.plan[k] is None:
                continue
            a = _tiles(p, k)
            assert a[:, 1].min() >= 1 and a[:, 1].max() <= tp.RMAX and a[:, 2].max() <= tp.UCAP
            assert a[:, 3].max() <= tp.ECAP and a[:, 4].max() <= tp.ECAP + 3 * tp.RMAX
            assert a[0, 0] == 0 and np.array_equal(a[1:, 0], np.cumsum(a[:-1, 1]))
            assert a[:, 1].sum() == (p.n_pair_real if k == 2 else p.n_real)


def test_restatement_reproduces_the_fixture_tile_counts():
    """The SMPL-like fixture, levels 0-2: 230 finest-level tiles is the figure csrc/capi.hip quotes for its locality order."""
    gL, _, _ = helpers.golden_graphs("human36")
    want = [(230, 216, 233), (123, 114, 128), (63, 61, 68)]
    for L, w in zip(gL[:3], want):
        p = tp.Plans(L)
        assert p.plan_tiles == w
        assert max(p.row_len[0]) <= 44 and p.summary(0)["one_row"] == 0      # what the network tests reach: far from the caps
