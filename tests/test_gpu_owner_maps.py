"""The multi-rank device path under the patch-to-rank map the reference itself uses (round-robin, Grid::DistributePatches) and three
other maps, on one device through the loopback hooks: k_pack and k_dss with their ghosts on up to three peers per group, the
boundary-first loop with nearly all tiles early or with ranks of one run in different modes, the early and late lists of the
node-unique layout, and the tracer, supercell, shallow-water and Rayleigh configurations over those lists.  Every case pairs ONE engine
that holds all patches with n rank engines built with owner=; the cases, their maps and what each is there for are
owner_maps_common.py's, qualified on the CPU by test_owner_maps_host.py.  (The real transport under the same map:
test_gpu_two_process.py.)"""
import numpy as np
import pytest

import golden_util as gu
import owner_maps_common as om
from parity_common import EXACT, UDIFF, _rank_engines_step, INFO_EARLY_TILES, INFO_LATE_TILES

pytestmark = pytest.mark.gpu

INFO_GHOST_COLUMNS, INFO_UNIQUE_LAYOUT, INFO_UNIQUE_INSTANCES = 4, 12, 13      # tmx_info (include/tempest_mi355x.h)


def _local(e, per_patch):
    return [per_patch[p] for p in e.local_patches]


def _identical(e, got, ref, gott=None, reft=None, sw=False):
    """The interior prognostic slots of the rank's patches, bit for bit (np.array_equal: a NaN on either side is a miss)."""
    for p in e.local_patches:
        slots = [0, 1, 2] if sw else [0, 1, 2, 4]
        assert np.array_equal(got[p][0][slots, 1:-1, 1:-1], ref[p][0][slots, 1:-1, 1:-1]), (e.rank, p)
        assert np.isfinite(ref[p][0][slots, 1:-1, 1:-1]).all(), (e.rank, p)
        if not sw:
            assert np.array_equal(got[p][1][3, 1:-1, 1:-1], ref[p][1][3, 1:-1, 1:-1]), (e.rank, p)
        if reft is not None:
            assert np.array_equal(gott[p][:, 1:-1, 1:-1], reft[p][:, 1:-1, 1:-1]), (e.rank, p)


# ---------------------------------------------------------------------------------------------
# a: the DSS and the pack on their own


@pytest.mark.parametrize("case", om.DSS_CASES, ids=om.case_id)
def test_dss_and_pack_of_rough_copies(case):
    """rough_copies on instance 0 of every rank engine, Engine.dss_loopback: on every rank's patches the result is the oracle's DSS bit for
    bit (all five variables, every tracer), and every scalar lies within 4 * 2**-53 * max |copies| of the long double mean of its copies,
    the groups found from the coordinates alone."""
    from tempestmodel_amd.engine import Engine
    from oracle_lib import Oracle
    g, states = om.grid_of(case)
    ntr, n = case["ntr"], case["ranks"]
    st, tr = om.rough_copies(states, ntr)
    o = Oracle(g); o.set_state(0, st)
    if ntr:
        o.set_tracers(0, tr)
    o.apply_dss(0)
    want, wantt = o.get_state(0), (o.get_tracers(0) if ntr else None)
    owner = om.owner_of(case)
    ranks = [Engine(g, rank=r, n_ranks=n, owner=owner) for r in range(n)]
    try:
        for e in ranks:
            assert e.info(INFO_GHOST_COLUMNS) > 0, e.rank
            e.upload_state(0, st)
            if ntr:
                e.upload_tracers(0, tr)
        Engine.dss_loopback(ranks, 0)
        full = [None] * case["npatch"]; fullt = [None] * case["npatch"]
        for e in ranks:
            e.sync()
            got = e.download_state(0)
            errs = gu.prognostic_errors(_local(e, got), _local(e, want))
            terrs = [0.0]
            if ntr:
                gott = e.download_tracers(0)
                terrs = gu.tracer_errors(_local(e, gott), _local(e, wantt))
            print("%s rank %d: against the oracle" % (om.case_id(case), e.rank), errs, terrs)
            assert max(errs) <= EXACT and max(terrs) <= EXACT, (e.rank, errs, terrs)
            for p in e.local_patches:
                full[p] = got[p]
                if ntr:
                    fullt[p] = gott[p]
        assert all(f is not None for f in full)
        nodes, group, count = om.groups_by_position(g)
        a = om.gather_nodes(om.column_vectors(st, tr), nodes)
        b = om.gather_nodes(om.column_vectors(full, fullt if ntr else None), nodes)
        d = om.distance_to_mean(b, a, nodes, group, count, om.scalar_entries(g.L, ntr))
        print("%s: device to long double mean, worst %.3f in units of 2**-53 * max|copies|" % (om.case_id(case), d))
        assert d <= om.MEAN_BOUND_ULPS, d
    finally:
        for e in ranks:
            e.close()


# ---------------------------------------------------------------------------------------------
# b, c: production steps behind the loopback wire


_references = {}


def _engine_kw(case):
    kw = {}
    if case["case"] == "smallplanet":
        kw.update(fully_explicit=True, uniform_diffusion=UDIFF)
    return kw


def _time_steps(case):
    """(dt of the compared steps, dt of the scrub step, number of compared steps)."""
    if case["case"] == "smallplanet":
        return 1.0, 0.5, 3
    if case["case"] == "schar":
        return 0.5, 0.3, 3
    if case["sw"]:
        return 200.0, 37.0, 5
    return 100.0, 37.0, 3


def _reference(case):
    """Once per case, shared by its layouts and left unchanged: the start state (one step of ONE engine from the pointwise initial state:
    developed, W != 0, copies consistent), that engine's state after the compared steps, and, where the case says so, the oracle's."""
    from tempestmodel_amd.engine import Engine
    from oracle_lib import Oracle
    key = om.case_id(case)
    if key in _references:
        return _references[key]
    g, states = om.grid_of(case)
    ntr, scheme = case["ntr"], case["scheme"]
    dt, _, nsteps = _time_steps(case)
    ni = max(5 if case["sw"] else 7, Engine.scheme_instances(scheme))
    tr0 = [g.initial_tracers[p] for p in range(case["npatch"])] if ntr else None
    single = Engine(g, n_instances=ni, **_engine_kw(case))
    try:
        single.upload_state(0, states)
        if ntr:
            single.upload_tracers(0, tr0)
        single.step(scheme, dt, first=True)
        single.sync()
        start, startt = single.download_state(0), (single.download_tracers(0) if ntr else None)
        single.upload_state(0, start)
        if ntr:
            single.upload_tracers(0, startt)
        for k in range(nsteps):
            single.step(scheme, dt, first=(k == 0))
        single.sync()
        ref, reft = single.download_state(0), (single.download_tracers(0) if ntr else None)
    finally:
        single.close()
    want = None
    if case.get("oracle"):
        o = Oracle(g, ninst=ni); o.set_state(0, start)
        for k in range(nsteps):
            assert o.step(scheme, dt, first=(k == 0)) == 0
        want = o.get_state(0)
        assert all(np.isfinite(n_).all() and np.isfinite(e_).all() for n_, e_ in want)
    _references[key] = (ni, tr0, start, startt, ref, reft, want)
    return _references[key]


def _run_ranks(case, options):
    """The rank engines of a case through one scrub step from the pointwise initial state with another dt (all ranks together: the step
    exchanges), then the compared steps from the start state; asserts the tile counts tmx_info reports against the plan's, the results
    against ONE engine bit for bit and against the oracle where the case carries one.  Returns the engines' UNIQUE_INSTANCES per rank."""
    from tempestmodel_amd.engine import Engine
    g, states = om.grid_of(case)
    ni, tr0, start, startt, ref, reft, want = _reference(case)
    n, scheme, ntr, sw = case["ranks"], case["scheme"], case["ntr"], case["sw"]
    dt, sdt, nsteps = _time_steps(case)
    owner = om.owner_of(case)
    tiles = om.predicted_tiles(case)
    ranks = [Engine(g, rank=r, n_ranks=n, owner=owner, n_instances=ni, options=options, **_engine_kw(case)) for r in range(n)]
    try:
        for e in ranks:
            assert e.info(INFO_GHOST_COLUMNS) > 0, e.rank
            if options:
                assert e.info(INFO_UNIQUE_LAYOUT) == options["unique_layout"], e.rank
            # the mode test_owner_maps_host.py predicted from the plan is the one this engine runs
            assert (e.info(INFO_EARLY_TILES), e.info(INFO_LATE_TILES)) == tiles[e.rank], (e.rank, e.info(INFO_EARLY_TILES), e.info(INFO_LATE_TILES), tiles)
            e.upload_state(0, states)
            if ntr:
                e.upload_tracers(0, tr0)
        Engine.loopback_group(ranks)
        _rank_engines_step(ranks, lambda e, k: e.step(scheme, sdt, first=True), 1)
        for e in ranks:
            e.upload_state(0, start)
            if ntr:
                e.upload_tracers(0, startt)
        _rank_engines_step(ranks, lambda e, k: e.step(scheme, dt, first=(k == 0)), nsteps)
        Engine.loopback_dissolve(ranks[0])
        unique = [e.info(INFO_UNIQUE_INSTANCES) for e in ranks]
        for e in ranks:
            got = e.download_state(0)
            gott = e.download_tracers(0) if ntr else None
            _identical(e, got, ref, gott, reft, sw=sw)
            if want is not None:
                errs = gu.prognostic_errors(_local(e, got), _local(e, want))
                print("%s %s rank %d: against the oracle" % (om.case_id(case), options, e.rank), errs)
                assert max(errs) <= EXACT, (e.rank, errs)
        print("%s %s: (early, late) per rank %s, node-unique instances per rank %s" % (om.case_id(case), options, tiles, unique))
        return tiles, unique
    finally:
        for e in ranks:
            e.close()


def _both(t):
    return t[0] > 0 and t[1] > 0


# unique_layout 0: element-major; 1: node-unique, default thread order; the mixed-split case also with the 2 x 2 thread order, whose tables
# give every rank both tile lists (a rank runs a node-unique stage boundary first only where its element-major plan splits as well)
LAYOUTS = [(c, {"unique_layout": 0}) for c in om.STEP_CASES] + [(c, {"unique_layout": 1}) for c in om.STEP_CASES] + [
    (om.CASE_MIXED_SPLIT, {"unique_layout": 1, "unique_tile_shape": 1})]


@pytest.mark.parametrize("case,options", LAYOUTS, ids=["%s-%s" % (om.case_id(c), "".join("%s%d" % (k[7], v) for k, v in o.items())) for c, o in LAYOUTS])
def test_production_steps(case, options):
    """tmx_step on the rank engines behind loopback_group, implicit vertical dynamics: three steps after a scrub step, bit-identical to one
    engine and, at ne <= 14, EXACT against the oracle stepped from the same state; element-major and node-unique; tmx_info says which tiles
    ran early and late on every rank and that the layout asked for is the one that ran."""
    tiles, unique = _run_ranks(case, options)
    if case is om.CASE_MIXED_SPLIT:      # ranks of one run in different modes of the boundary-first loop
        assert any(_both(t) for t in tiles) and any(t == (0, 0) for t in tiles), tiles
    else:
        assert all(_both(t) for t in tiles), tiles
    if case is om.CASE_TWO_LATE_TILES:
        assert min(t[1] for t in tiles) <= 2, tiles
    if not options["unique_layout"]:
        assert all(u == 0 for u in unique), unique
    elif case["scheme"] == "ark232":
        # StepImplicitTermsExplicitly has a node-unique form only where the metric copies of every node of the rank agree bit for bit
        # (UniqueLayout::vite_ok); either way is right, the results above are the proof
        print("ark232 ran node-unique on ranks", [r for r, u in enumerate(unique) if u > 0])
    else:
        assert all(u > 0 for u in unique), unique


@pytest.mark.parametrize("case", om.OTHER_CASES, ids=om.case_id)
def test_other_configurations_under_the_reference_map(case):
    """Two tracers; the supercell configuration (fully explicit vertical mode, uniform diffusion, two tracers, Strang); shallow water (five
    Strang steps); a Rayleigh layer (tmx_set_patch_rayleigh is per owned patch, the relaxation per stored copy): bit-identical to one
    engine, every rank with early and late tiles."""
    assert case["map"] == "reference"
    tiles, unique = _run_ranks(case, None)
    assert all(_both(t) for t in tiles), tiles
