"""CPU qualification of the cases test_gpu_owner_maps.py runs on the device (owner_maps_common.py): for every case, on plan-only
engines, the wire lists of every pair of ranks agree entry by entry, the exchange plan executed in numpy reproduces the oracle's DSS of
a state whose stored copies all differ bit for bit (tracers included), and that DSS is the mean of the copies within the bound the
kernel's operation order gives against a long double mean over groups found from the coordinates alone.  The last test restates from the
plan what each case is in the tables for (tiles early and late per rank in both layouts, groups by number of owning ranks, unequal
patch counts, a rank with a quarter of a tile): if a table entry stops showing its feature it fails here, and the GPU file does not
change.  Run with -s to read the figures."""
import numpy as np
import pytest

import owner_maps_common as om
from oracle_lib import Oracle


def _key(c):
    """A case without its time scheme: what the plan depends on."""
    return om.case_id({k: v for k, v in c.items() if k != "scheme"})


def _distinct(cases):
    seen, out = set(), []
    for c in cases:
        k = _key(c)
        if k not in seen:
            seen.add(k); out.append(c)
    return out


CASES = _distinct(om.ALL_CASES)
DSS_ABLE = [c for c in CASES if not c["sw"]]


def _engines(case):
    g, states = om.grid_of(case)
    owner = om.owner_of(case)
    assert sorted(set(owner)) == list(range(case["ranks"])), owner      # every rank owns a patch
    return g, states, owner, om.plan_engines(g, owner, case["ranks"])


@pytest.mark.parametrize("case", CASES, ids=om.case_id)
def test_wire_lists_agree(case):
    """Rank s's send list to d is d's receive list from s, entry by entry in (patch, i, j); every rank sends and receives (a rank with
    neither would leave the exchange out, and with it the loopback barrier the others wait at)."""
    g, _, owner, engines = _engines(case)
    try:
        tabs = [om.plan_tables(e) for e in engines]
        for d, td in enumerate(tabs):
            assert len(td["send"]) > 0 and len(td["recv"]) > 0, d
            assert all(owner[p] == d for p in td["send"][:, 0]) and all(owner[p] != d for p in td["recv"][:, 0]), d
            for s, ts in enumerate(tabs):
                if s == d:
                    assert not (td["send"][:, 3] == d).any() and not (td["recv"][:, 3] == d).any()
                    continue
                out = ts["send"][ts["send"][:, 3] == d][:, :3]
                inn = td["recv"][td["recv"][:, 3] == s][:, :3]
                assert np.array_equal(out, inn), (s, d, len(out), len(inn))
        print("%s: columns sent per rank %s" % (om.case_id(case), [len(t["send"]) for t in tabs]))
    finally:
        for e in engines:
            e.close()


_oracle_dss = {}


def _rough_and_oracle(case):
    """rough_copies of the case and the oracle's DSS of it, as column vectors; computed once per case and left unchanged."""
    k = _key(case)
    if k not in _oracle_dss:
        g, states = om.grid_of(case)
        st, tr = om.rough_copies(states, case["ntr"])
        o = Oracle(g); o.set_state(0, st)
        if tr is not None:
            o.set_tracers(0, tr)
        o.apply_dss(0)
        _oracle_dss[k] = (om.column_vectors(st, tr), om.column_vectors(o.get_state(0), o.get_tracers(0) if tr is not None else None))
    return _oracle_dss[k]


@pytest.mark.parametrize("case", DSS_ABLE, ids=om.case_id)
def test_plan_reproduces_the_oracle(case):
    """The plan of every rank executed in numpy on rough_copies (the ghost buffer filled from the SENDERS' lists, in wire order) equals
    Oracle.apply_dss on every local member of every group: worst difference == 0.0, all five variables and every tracer."""
    g, _, owner, engines = _engines(case)
    try:
        vin, vout = _rough_and_oracle(case)
        tabs = [om.plan_tables(e) for e in engines]
        worst, seen = 0.0, 0
        for d, td in enumerate(tabs):
            ghost = np.full((len(td["recv"]), vin[0].shape[-1]), np.nan)
            for s, ts in enumerate(tabs):
                rows = ts["send"][ts["send"][:, 3] == d]
                if s != d and len(rows):      # (under the block map some pairs of ranks share no node)
                    ghost[td["recv"][:, 3] == s] = np.array([vin[p][i, j] for p, i, j, _ in rows]).reshape(len(rows), -1)
            for (p, i, j), res in om.execute_plan(td, om.column_lookup(g, owner, d), g.L, lambda p, i, j: vin[p][i, j], ghost):
                x = float(np.max(np.abs(res - vout[p][i, j])))
                worst = x if not np.isfinite(x) or x > worst else worst      # (a NaN is kept and fails `== 0.0`)
                seen += 1
        nodes, group, count = om.groups_by_position(g)
        assert seen == int((count[group] >= 2).sum()), (seen, int((count[group] >= 2).sum()))      # every stored copy of every shared node, once
        print("%s: plan against oracle, worst absolute difference %g over %d copies" % (om.case_id(case), worst, seen))
        assert worst == 0.0, worst
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("case", _distinct([dict(c, ranks=0, map="") for c in DSS_ABLE]), ids=lambda c: _key(c).split("-r0")[0])
def test_oracle_dss_is_the_mean_of_the_copies(case):
    """Oracle.apply_dss on rough_copies against mean_longdouble over groups_by_position, per node and entry within 4 * 2**-53 * max |copies|
    on every scalar (rho*theta, rho, W on interfaces, each tracer) and on U, V where all copies lie on one panel.  Groups come out with 2,
    3 and 4 copies, exactly 8 of them with 3 (the cube's corners)."""
    g, _ = om.grid_of(case)
    vin, vout = _rough_and_oracle(case)
    nodes, group, count = om.groups_by_position(g)
    assert set(np.unique(count)) == {1, 2, 3, 4} and int((count == 3).sum()) == 8, np.unique(count, return_counts=True)
    assert len(nodes) == 16 * 6 * case["ne"] ** 2
    a, b = om.gather_nodes(vin, nodes), om.gather_nodes(vout, nodes)
    L = g.L
    ds = om.distance_to_mean(b, a, nodes, group, count, om.scalar_entries(L, case["ntr"]))
    dv = om.distance_to_mean(b, a, nodes, group, count, np.arange(2 * L), panels=[P.panel for P in g.patches])
    print("ne%d L%d %d patches, %d tracers: oracle to long double mean, worst %.3f (scalars) %.3f (U, V inside a panel) in units of 2**-53 * max|copies|"
          % (case["ne"], L, case["npatch"], case["ntr"], ds, dv))
    assert ds <= om.MEAN_BOUND_ULPS and dv <= om.MEAN_BOUND_ULPS, (ds, dv)
    assert ds > 0.0      # (the state is rough: a mean that needed no rounding anywhere would mean the copies agree)


def _tiles(case):
    g, _, owner, engines = _engines(case)
    try:
        em = [om.element_major_tiles(e) for e in engines]
        nu = {shape: [om.node_unique_tiles(e, shape) for e in engines] for shape in (0, 1)}
        cols = [int(e.plan(3)[1]) for e in engines]
    finally:
        for e in engines:
            e.close()
    return g, owner, em, nu, cols


def test_cases_hold_what_they_are_there_for():
    """Per case: early and late tiles per rank, element-major (tmx_plan_get 7, 8) and node-unique (tmx_debug_unique_tables, the default tile
    shape 0 and the 2 x 2 shape 1), and the groups by copies and owning ranks; then the features the tables name."""
    facts = {}
    for case in CASES:
        g, owner, em, nu, cols = _tiles(case)
        census = om.census_by_owning_ranks(g, owner)
        npat = [owner.count(r) for r in range(case["ranks"])]
        facts[_key(case)] = (em, nu, census, npat, cols)
        print("%s:\n   patches per rank %s, stored columns %s\n   element-major (early, late) %s\n   node-unique shape 0 %s\n   node-unique shape 1 %s\n"
              "   groups {(copies, owning ranks): count} %s" % (om.case_id(case), npat, cols, em, nu[0], nu[1], dict(sorted(census.items()))))

    def of(case):
        return facts[_key(case)]

    def both(t):
        return t[0] > 0 and t[1] > 0
    # under `reference`, every rank with early and late tiles in both layouts
    em, nu, _, _, _ = of(om.CASE_BOTH_KINDS_OF_TILES)
    assert om.CASE_BOTH_KINDS_OF_TILES["map"] == "reference" and all(both(t) for t in em) and all(both(t) for t in nu[0]) and all(both(t) for t in nu[1])
    # a rank with no more than 2 late tiles
    em, nu, _, _, _ = of(om.CASE_TWO_LATE_TILES)
    assert om.CASE_TWO_LATE_TILES["map"] == "reference" and all(both(t) for t in em) and min(t[1] for t in em) <= 2
    # element-major: some ranks split, others do not; the node-unique tables of the 2 x 2 shape have both lists on every rank
    em, nu, _, _, _ = of(om.CASE_MIXED_SPLIT)
    assert om.CASE_MIXED_SPLIT["map"] == "reference" and any(both(t) for t in em) and any(t == (0, 0) for t in em) and all(both(t) for t in nu[1])
    # groups of four on four ranks and ALL eight cube corners on three (the DSS on its own); the step cases see both kinds as well (four
    # of the corners at ne12 on 4 ranks) -- and under the block map of that grid and rank count no group spans more than three ranks
    _, _, census, _, _ = of(om.CASE_FOUR_RANKS_PER_GROUP)
    assert census.get((4, 4), 0) > 0 and census.get((3, 3), 0) == 8, census
    c = om.CASE_TWO_LATE_TILES
    _, _, census, _, _ = of(c)
    assert census.get((4, 4), 0) > 0 and census.get((3, 3), 0) > 0, census
    blk = om.census_by_owning_ranks(om.grid_of(c)[0], om.block(c["npatch"], c["ranks"]))
    assert (4, 4) not in blk and max(r for _, r in blk) <= 3, blk
    # unequal patch counts
    _, _, _, npat, _ = of(om.CASE_UNEQUAL_PATCH_COUNTS)
    assert sorted(set(npat)) == [7, 8], npat
    # a rank with less than a tile of columns: 16, a quarter
    _, _, _, npat, cols = of(om.CASE_LESS_THAN_A_TILE)
    assert npat[0] == 1 and cols[0] == 16, (npat, cols)
    # the block-map case of the DSS table has unequal blocks
    _, _, _, npat, _ = of(om.DSS_CASES[7])
    assert om.DSS_CASES[7]["map"] == "block" and len(set(npat)) > 1, npat
    # every rank of every case has ghost columns and columns to send (test_wire_lists_agree), so every rank takes part in every exchange


def test_owner_maps_are_what_they_say():
    assert om.reference(7, 3) == [0, 1, 2, 0, 1, 2, 0]
    assert om.lone_patch(24, 2) == [0] + [1] * 23 and om.lone_patch(24, 4).count(0) == 1
    s = om.OWNER_MAPS["shuffled"](24, 4)
    assert sorted(s) == sorted(om.reference(24, 4)) and s != om.reference(24, 4) and s != om.block(24, 4)
    assert s == om.OWNER_MAPS["shuffled"](24, 4)      # fixed
    strides = {b - a for r in range(4) for a, b in zip([p for p in range(24) if s[p] == r], [p for p in range(24) if s[p] == r][1:])}
    assert len(strides) > 2      # neither contiguous nor strided
