"""DCMIPPhysics::Perform on the device (tmx_physics_dcmip2016) against the reference's own results: the DCMIP2016 tropical
cyclone (test 2) and moist baroclinic wave (test 1, 5 tracers), every (pbl, prec) variant and test 3, per call and across steps.
exp / pow are glibc's restated bit for bit (tmx_refmath.h), sqrt is IEEE, the covector coefficients and Tsurf come from the
host's libm: state, tracers and precipitation are the reference's doubles."""
import numpy as np
import pytest
import golden_util as gu
import dcmip_common as dc

pytestmark = pytest.mark.gpu

CASES = [("tc", 2, 3), ("bw", 1, 5)]


def _setup(case, ntracers, **kw):
    from tempestmodel_amd.engine import Engine
    d = dc.load_case(case)
    g, _ = gu.grid_from_fixture(d, ntracers=ntracers)
    e = Engine(g, **kw)
    zl, zi = zip(*[dc.heights(d, P) for P in g.patches])
    e.set_level_heights(list(zl))
    e.set_dcmip_inputs(latitude=[d["p%d/lat" % P.index] for P in g.patches], a_nodes=[d["p%d/a_nodes" % P.index] for P in g.patches],
                       b_nodes=[d["p%d/b_nodes" % P.index] for P in g.patches], z_interfaces=list(zi),
                       earth_radius=float(d["phys/earth_radius"][0]))
    return d, g, e


def _upload(e, d, g, tag):
    e.upload_state(0, gu.expand_compact(d, tag, g))
    e.upload_tracers(0, gu.expand_compact_tracers(d, tag, g))


def _check_call(e, d, g, start, call):
    """The device state after a call against the fixture, == 0.0 everywhere (W and tracers 3+ against the starting state).  Every pair
    goes through golden_util's own per-pair function: a value that is not finite, on either side, makes the result inf and fails the
    caller's `== 0.0` (Python's max(0.0, nan) is 0.0, which would let a NaN result pass), and a pair of unequal shapes raises."""
    got, gt = e.download_state(0), e.download_tracers(0)
    prect = e.download_precipitation(reset=True)
    worst = 0.0

    def fold(worst, a, b):
        return gu.worse(worst, gu._pair(a, b)[0])
    for P in g.patches:
        p = P.index
        n, w = got[p]
        worst = fold(worst, n[[0, 1, 2, 4], 1:-1, 1:-1], dc.decode_after(d, start, call, p, "node"))
        worst = fold(worst, w[3, 1:-1, 1:-1], d["state/%s/p%d/redge" % (start, p)])
        t = gt[p][:, 1:-1, 1:-1]
        worst = fold(worst, t[:3], dc.decode_after(d, start, call, p, "tracers"))
        if t.shape[0] > 3:
            worst = fold(worst, t[3:], d["state/%s/p%d/tracers" % (start, p)][3:])
        worst = fold(worst, prect[p][1:-1, 1:-1], d["prect/%s/p%d" % (call, p)][1:-1, 1:-1])
    return worst


@pytest.mark.parametrize("case,test,ntracers", CASES)
@pytest.mark.parametrize("lds", [0, 1])
def test_dcmip_physics_per_call_matches_the_reference(case, test, ntracers, lds):
    """lds: the Thomas coefficients in LDS (option dcmip_lds) instead of the HBM work arrays."""
    d, g, e = _setup(case, ntracers, options={"dcmip_lds": lds})
    dt = float(d["cfg/dt"][0])
    try:
        for start in ("stock", "warm", "moist"):
            calls = [(test, pb, pr) for pb, pr in dc.COMBOS] + [(3, 0, 0)]
            for t, pb, pr in calls:
                _upload(e, d, g, start)
                e.download_precipitation(reset=True)
                e.dcmip2016(0, dt, t, pb, pr)
                e.sync()
                call = "%s_t%d_pbl%d_prec%d" % (start, t, pb, pr)
                worst = _check_call(e, d, g, start, call)
                print(call, "max |device - reference| =", worst)
                assert worst == 0.0, (call, worst)
    finally:
        e.close()


@pytest.mark.parametrize("pbl,prec", [(0, 0), (1, 1)])
def test_tropical_cyclone_steps_with_dcmip_physics(pbl, prec):
    """Three ARS343 steps of the tropical cyclone, DCMIPPhysics::Perform after every step (Model.cpp:470-481), against the
    reference's state, from the state after the same two warm-up steps."""
    s = gu.load("dcmip_tc_steps_%s.npz" % dc.GRID)
    d, g, e = _setup("tc", 3)
    dt = float(s["cfg/dt"][0])
    try:
        _upload(e, d, g, "warm")          # the warm state is stored once, with the per-call data
        for _ in range(3):
            e.step_ars343(dt)
            e.dcmip2016(0, dt, 2, pbl, prec)
        e.sync()
        got, gt = e.download_state(0), e.download_tracers(0)
        worst = 0.0
        for p in range(6):
            for what in ("node", "redge", "tracers"):
                base = np.ascontiguousarray(d["state/warm/p%d/%s" % (p, what)])
                ref = np.bitwise_xor(base.view(np.uint64), s["xor/pbl%d_prec%d_step3/p%d/%s" % (pbl, prec, p, what)]).view(np.float64)
                have = {"node": got[p][0][[0, 1, 2, 4], 1:-1, 1:-1], "redge": got[p][1][3, 1:-1, 1:-1], "tracers": gt[p][:, 1:-1, 1:-1]}[what]
                worst = gu.worse(worst, gu._fold([(have, ref)], floor=1e-300))
        print("steps pbl %d prec %d: max relative difference vs reference %.3e" % (pbl, prec, worst))
        assert worst <= gu.exact_tolerance(), worst
    finally:
        e.close()


def test_node_unique_and_element_major_instances_give_the_same_bits():
    """An instance the step left node-unique is converted the way tmx_physics_kessler converts it: the physics sees the same
    columns and writes the same bits as on the element-major engine."""
    from tempestmodel_amd.engine import Engine
    d, g, e = _setup("tc", 3, options={"unique_layout": 1})
    d, g, e2 = _setup("tc", 3, options={"unique_layout": 0})
    dt = float(d["cfg/dt"][0])
    try:
        outs = []
        for eng in (e, e2):
            _upload(eng, d, g, "moist")
            eng.step_ars343(dt)
            eng.dcmip2016(0, dt, 2, 1, 0)
            eng.sync()
            outs.append((eng.download_state(0), eng.download_tracers(0), eng.download_precipitation()))
        for p in range(6):
            assert np.array_equal(outs[0][0][p][0], outs[1][0][p][0]), p
            assert np.array_equal(outs[0][1][p], outs[1][1][p]), p
            assert np.array_equal(outs[0][2][p], outs[1][2][p]), p
    finally:
        e.close(); e2.close()


def test_dcmip_physics_errors_leave_the_state_alone():
    from tempestmodel_amd.engine import Engine, TempestError
    d = dc.load_case("tc")
    g, _ = gu.grid_from_fixture(d, ntracers=3)
    e = Engine(g)
    try:
        _upload(e, d, g, "moist")
        with pytest.raises(TempestError) as ex:
            e.dcmip2016(0, 300.0, 2, 1, 1)                 # inputs not set
        assert ex.value.code == -1
        zl, zi = zip(*[dc.heights(d, P) for P in g.patches])
        e.set_level_heights(list(zl))
        with pytest.raises(TempestError) as ex:
            e.dcmip2016(0, 300.0, 2, 1, 1)                 # level heights only
        assert ex.value.code == -1
        e.set_dcmip_inputs(latitude=[d["p%d/lat" % P.index] for P in g.patches], a_nodes=[d["p%d/a_nodes" % P.index] for P in g.patches],
                           b_nodes=[d["p%d/b_nodes" % P.index] for P in g.patches], z_interfaces=list(zi))
        for args in ((0, 300.0, 0, 1, 1), (0, 300.0, 4, 1, 1), (0, 300.0, 2, 2, 1), (0, 300.0, 2, -1, 1), (0, 300.0, 2, 1, 2),
                     (0, 300.0, 2, 1, -1), (0, 0.0, 2, 1, 1), (0, -300.0, 2, 1, 1), (99, 300.0, 2, 1, 1)):
            with pytest.raises(TempestError) as ex:
                e.dcmip2016(*args)
            assert ex.value.code == -1, args
        e.sync()
        got, gt = e.download_state(0), e.download_tracers(0)
        ref = gu.expand_compact(d, "moist", g)
        for p in range(6):
            assert np.array_equal(got[p][0][[0, 1, 2, 4], 1:-1, 1:-1], ref[p][0][[0, 1, 2, 4], 1:-1, 1:-1])
            assert np.array_equal(gt[p][:, 1:-1, 1:-1], d["state/moist/p%d/tracers" % p])
        assert all(float(np.max(np.abs(v))) == 0.0 for v in e.download_precipitation().values())
    finally:
        e.close()
    # fewer than three tracers
    g0, _ = gu.grid_from_fixture(d, ntracers=0)
    e0 = Engine(g0)
    try:
        zl, zi = zip(*[dc.heights(d, P) for P in g0.patches])
        e0.set_level_heights(list(zl))
        e0.set_dcmip_inputs(latitude=[d["p%d/lat" % P.index] for P in g0.patches], z_interfaces=list(zi))
        with pytest.raises(TempestError) as ex:
            e0.dcmip2016(0, 300.0, 2, 1, 1)
        assert ex.value.code == -1
    finally:
        e0.close()
    # the shallow-water equation set
    from tempestmodel_amd.cubed_sphere import CubedSphereGrid, ShallowWaterTest2
    gs = CubedSphereGrid(4, 1, 1.0, shallow_water=True)
    gs.evaluate_test_case(ShallowWaterTest2())
    es = Engine(gs, n_instances=5)
    try:
        with pytest.raises(TempestError) as ex:
            es.dcmip2016(0, 300.0, 2, 1, 1)
        assert ex.value.code == -2
    finally:
        es.close()
