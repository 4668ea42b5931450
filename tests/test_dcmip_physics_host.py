"""DCMIP2016 column physics (tmx_physics_dcmip2016), the parts that run without a GPU: the per-node covector coefficients the host
forms at set-up against a plain restatement of the reference's transforms, and what the reference fixtures must show to be
worth pinning."""
import ctypes as C
import math
import numpy as np
import pytest
import golden_util as gu
import dcmip_common as dc

PD = C.POINTER(C.c_double)


def _lib():
    from tempestmodel_amd.engine import load_library
    return load_library()


def _coefficients(lib, panel, a, b):
    out = np.zeros(11)
    assert lib.tmx_debug_dcmip_node_coefficients(panel, a, b, out.ctypes.data_as(PD)) == 0
    return out


def _apply_rll(c, ua, ub):
    return (c[0] * ua + c[1] * ub) * c[4], c[2] * ua + c[3] * ub


def _apply_abp(c, ulon, ulat):
    lon = ulon / c[5]
    return c[6] * lon + c[7] * ulat, c[8] * lon + c[9] * ulat


def test_covector_coefficients_match_the_reference_transforms():
    """Both directions on all six panels, at GLL-like and random angles, the polar panel centres (|X|, |Y| < 1e-13) included:
    coefficient x component products give the reference's doubles bit for bit (0.0 == -0.0 where a term is absent)."""
    lib = _lib()
    rng = np.random.default_rng(7)
    angles = list(rng.uniform(-math.pi / 4, math.pi / 4, size=(40, 2)))
    angles += [(0.0, 0.0), (1e-14, -3e-14), (0.0, 0.3), (-0.2, 0.0), (math.pi / 4, -math.pi / 4)]
    n = 0
    for panel in range(6):
        for a, b in angles:
            c = _coefficients(lib, panel, float(a), float(b))
            X, Y = math.tan(a), math.tan(b)
            for ua, ub in rng.normal(scale=30.0, size=(4, 2)):
                got = _apply_rll(c, float(ua), float(ub))
                ref = dc.rll_from_abp(X, Y, panel, float(ua), float(ub))
                assert got[0] == ref[0] and got[1] == ref[1], (panel, a, b, got, ref)
                got2 = _apply_abp(c, ref[0], ref[1])
                ref2 = dc.abp_from_rll(X, Y, panel, ref[0], ref[1])
                assert got2[0] == ref2[0] and got2[1] == ref2[1], (panel, a, b, got2, ref2)
                # round trip: back to the components within rounding
                assert abs(got2[0] - ua) <= 1e-12 * (abs(ua) + abs(ub)) and abs(got2[1] - ub) <= 1e-12 * (abs(ua) + abs(ub))
                n += 1
    assert n == 6 * len(angles) * 4
    # the panel-centre branch of the polar panels is the identity up to the sign of u_lon
    c4, c5 = _coefficients(lib, 4, 0.0, 0.0), _coefficients(lib, 5, 0.0, 0.0)
    assert list(c4[:10]) == [1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0]
    assert list(c5[:10]) == [-1.0, 0.0, 0.0, 1.0, 1.0, 1.0, -1.0, 0.0, 0.0, 1.0]
    assert lib.tmx_debug_dcmip_node_coefficients(6, 0.0, 0.0, np.zeros(11).ctypes.data_as(PD)) != 0


def test_test1_surface_temperature_is_the_moist_baroclinic_wave_profile():
    """Tsurf of test 1 (dcmip_physics_z_v1.f90:204-212) as the host forms it, against the source expression evaluated in
    Python (the folded constants of the compiled Fortran may move the last bit, nothing more)."""
    lib = _lib()
    lib.tmx_debug_dcmip_tsurf.argtypes = [C.c_double, PD]
    pi = 4.0 * math.atan(1.0)
    T00, u0, rair, a, omega, q0 = 288.0, 35.0, 287.0, 6371220.0, 7.29212e-5, 0.021
    latw, eta0 = 2.0 * pi / 9.0, 0.252
    etav = (1.0 - eta0) * 0.5 * pi
    zvir = (461.5 / 287.0) - 1.0
    for lat in np.linspace(-1.5, 1.5, 61):
        s, c = math.sin(lat), math.cos(lat)
        ref = (T00 + pi * u0 / rair * 1.5 * math.sin(etav) * math.cos(etav) ** 0.5 *
               ((-2.0 * s ** 6 * (c ** 2 + 1.0 / 3.0) + 10.0 / 63.0) * u0 * math.cos(etav) ** 1.5 +
                (8.0 / 5.0 * c ** 3 * (s ** 2 + 2.0 / 3.0) - pi / 4.0) * a * omega * 0.5)) / (1.0 + zvir * q0 * math.exp(-(lat / latw) ** 4))
        out = C.c_double()
        assert lib.tmx_debug_dcmip_tsurf(float(lat), C.byref(out)) == 0
        assert abs(out.value - ref) <= 4e-14 * ref, (lat, out.value, ref)


@pytest.mark.parametrize("case,test", [("tc", 2), ("bw", 1)])
def test_fixtures_exercise_every_branch(case, test):
    """The moistened starting state makes every branch act (RJ supersaturation, Kessler precipitation, lowest-level wind on
    both sides of 20 m/s, presi and zi on both sides of pbltop and zpbltop, an interface inside the Bryan boundary layer where
    its diffusivity is not zero), and the fixtures tell the variants apart."""
    d = dc.load_case(case)
    for k, v in d.items():
        if k.startswith("branches/moist/"):
            assert int(v[0]) > 0, k
    def after(call, p, what):
        return dc.decode_after(d, "moist", call, p, what)
    for p in range(6):
        base = "moist_t%d_pbl%%d_prec%%d" % test
        assert not np.array_equal(after(base % (0, 0), p, "node"), after(base % (1, 0), p, "node"))
        assert not np.array_equal(after(base % (0, 0), p, "tracers"), after(base % (0, 1), p, "tracers"))
        # test 3 (supercell) skips the boundary layer: it differs from test `test` with the same precipitation
        assert not np.array_equal(after("moist_t3_pbl0_prec0", p, "node"), after(base % (0, 0), p, "node"))
    pr0 = sum(float(np.sum(d["prect/moist_t%d_pbl0_prec0/p%d" % (test, p)])) for p in range(6))
    pr1 = sum(float(np.sum(d["prect/moist_t%d_pbl0_prec1/p%d" % (test, p)])) for p in range(6))
    assert pr0 > 0.0 and pr1 > 0.0 and pr0 != pr1


def test_moist_baroclinic_wave_leaves_the_chemistry_tracers_alone():
    """BaroclinicWaveUMJSTest carries 5 tracers; DCMIPPhysics::Perform writes only the first three.  The generator checks
    tracers 3 and 4 bit for bit and leaves them out of the stored results: here the starting states carry them and they are
    not all zero, so the check was not vacuous."""
    d = dc.load_case("bw")
    for start in ("stock", "warm", "moist"):
        tr = d["state/%s/p0/tracers" % start]
        assert tr.shape[0] == 5 and np.any(tr[3:] != 0.0)
        assert d["xor/%s_t1_pbl0_prec0/p0/tracers" % start].shape[0] == 3


# which branch counters each slim file leaves at zero (everything else is > 0); asserted exactly below
SLIM_MISSES = {
    ("A", "tc"): set(),
    ("B", "tc"): {"wind_above_20_columns"},
    ("B", "bw"): {"wind_below_20_columns"},
    ("Bp", "tc"): {"wind_above_20_columns"},
    ("C", "tc"): {"wind_above_20_columns"},
    ("D", "tc"): {"wind_above_20_columns", "zi_inside_bryan_pbl_interfaces"},
    ("D", "bw"): {"wind_below_20_columns", "zi_inside_bryan_pbl_interfaces"},
    ("E", "tc"): {"wind_above_20_columns", "zi_le_zpbltop_interfaces", "zi_inside_bryan_pbl_interfaces"},
}


@pytest.mark.parametrize("sid,case", dc.SLIM_FILES, ids=dc.SLIM_IDS)
def test_slim_fixtures_are_worth_pinning(sid, case):
    """The slim fixtures at the further shapes (dcmip_common.SLIM): every array finite; a column count that is no multiple of 64
    (864 = 13.5 workgroups at ne3, 96 = 1.5 at ne1); every recorded call differs from the starting state on every patch; the four
    (pbl, prec) results differ pairwise and test 3 differs from the file's own test with the same options; the baroclinic wave's
    tracers 3 and 4 are not all zero.

    A alone reaches both sides of every branch.  The ne1 grids do not, one file at a time -- 96 columns of one case lie on one side
    of 20 m/s: the tropical cyclone has no column above it, the baroclinic wave none below, so B and D reach both sides only with
    their two cases together (asserted), and B', C and E, which have the tropical cyclone alone, run the wind < 20 m/s side only.
    D (30 levels in 30 km, production's) has its lowest interior interface at 1 km: none lies strictly inside the Bryan layer, which
    is the branch mix production runs.  E (4 levels of 1125 m; the reference's column solve refuses 3) has no interior interface at
    or below 1 km either.  SLIM_MISSES holds exactly this, and is asserted as an equality."""
    d = dc.load_slim(sid, case)
    ne, L, ztop, dt, _ = dc.SLIM[sid]
    assert (int(d["cfg/ne"][0]), int(d["cfg/levels"][0]), float(d["cfg/ztop"][0]), float(d["cfg/dt"][0])) == (ne, L, float(ztop), float(dt))
    for k, v in d.items():
        if v.dtype == np.float64:
            assert np.all(np.isfinite(v)), k
    ncol = sum(d["state/moist/p%d/node" % p].shape[1] * d["state/moist/p%d/node" % p].shape[2] for p in range(6))
    assert ncol == 96 * ne * ne and ncol % 64 != 0, ncol
    assert not any(k.startswith(("state/stock", "state/warm", "op/", "grid/", "halo_trans/")) or "metric" in k or "jacobian" in k for k in d)
    calls = [dc.call_key(*c) for c in dc.slim_calls(d)]
    test = dc.slim_test(d)
    assert test == (2 if case == "tc" else 1)
    for p in range(6):
        res = {}
        for call in calls:
            assert np.any(d["xor/%s/p%d/node" % (call, p)] != 0) and np.any(d["xor/%s/p%d/tracers" % (call, p)] != 0), (call, p)
            res[call] = np.concatenate([dc.decode_after(d, "moist", call, p, "node").ravel(), dc.decode_after(d, "moist", call, p, "tracers").ravel()])
        four = calls[:4]
        for i in range(4):
            for j in range(i + 1, 4):
                assert not np.array_equal(res[four[i]], res[four[j]]), (four[i], four[j], p)
        assert not np.array_equal(res["moist_t3_pbl0_prec0"], res[dc.call_key(test, 0, 0)]), p
        if case == "bw":
            tr = d["state/moist/p%d/tracers" % p]
            assert tr.shape[0] == 5 and np.any(tr[3] != 0.0) and np.any(tr[4] != 0.0), p
    for pr_ in (0, 1):
        assert sum(float(np.sum(d["prect/%s/p%d" % (dc.call_key(test, 0, pr_), p)])) for p in range(6)) > 0.0
    zero = {k.split("/")[-1] for k, v in d.items() if k.startswith("branches/moist/") and int(v[0]) == 0}
    assert len([k for k in d if k.startswith("branches/moist/")]) == 10
    assert zero == SLIM_MISSES[(sid, case)], zero


def test_slim_ne1_cases_reach_both_wind_branches_jointly():
    """B and D: the tropical cyclone and the baroclinic wave together leave no counter at zero but D's `inside the Bryan layer`."""
    for sid, allowed in (("B", set()), ("D", {"zi_inside_bryan_pbl_interfaces"})):
        assert SLIM_MISSES[(sid, "tc")] & SLIM_MISSES[(sid, "bw")] == allowed, sid
    assert not SLIM_MISSES[("A", "tc")]


def test_checkerboard_partners_differ_at_every_column():
    """B and B' (same grid, level count and dt; tops of 12 and 4.5 km) share latitude and node angles and differ in every level and
    interface height above the ground and, at every column, in the starting state and in every recorded result: a checkerboard of the
    two (tests/test_gpu_dcmip_levels.py) puts different heights and different states into neighbouring lanes."""
    b, bp = dc.load_slim("B"), dc.load_slim("Bp")
    assert float(b["cfg/dt"][0]) == float(bp["cfg/dt"][0])
    for p in range(6):
        for nm in ("lat", "a_nodes", "b_nodes"):
            assert np.array_equal(b["p%d/%s" % (p, nm)], bp["p%d/%s" % (p, nm)]), (p, nm)
        assert np.all(b["p%d/dcmip_z_levels" % p] != bp["p%d/dcmip_z_levels" % p])
        assert np.all(b["p%d/dcmip_z_interfaces" % p][1:] != bp["p%d/dcmip_z_interfaces" % p][1:])
        for what in ("node", "tracers"):
            x, y = b["state/moist/p%d/%s" % (p, what)], bp["state/moist/p%d/%s" % (p, what)]
            assert np.all(np.any(x != y, axis=(0, 3))), (p, what)
            for call in (dc.call_key(*c) for c in dc.slim_calls(b)):
                x, y = dc.decode_after(b, "moist", call, p, what), dc.decode_after(bp, "moist", call, p, what)
                assert np.all(np.any(x != y, axis=(0, 3))), (p, what, call)


def test_kessler_subcycles_differ_inside_the_first_wavefront_of_A():
    """levels_common.kessler_subcycles (an estimate of the rain loop's sub-cycle count, float64 throughout) on A's moist state with A's
    heights and dt: the 64 columns of the first wavefront of k_dcmip hold more than one count, so lanes leave the loop at different
    trips.  (k_dcmip's Kessler works on the state the subroutine derives -- dry density, the clamped mixing ratios --, the same
    quantities the estimate forms.)"""
    import levels_common as lc
    d = dc.load_slim("A")
    g = dc.slim_grid(d)
    states, tracers, saved = gu.expand_compact(d, "moist", g), gu.expand_compact_tracers(d, "moist", g), []
    for P in g.patches:
        saved.append(P.geom["z_levels"])
        P.geom["z_levels"] = dc.heights(d, P)[0]
    try:
        with np.errstate(divide="ignore", invalid="ignore"):
            n = lc.kessler_subcycles(g, states, tracers, float(d["cfg/dt"][0]))
    finally:
        for P, z in zip(g.patches, saved):
            P.geom["z_levels"] = z
    first = sorted(set(int(v) for v in n[:64]))
    print("A: rain sub-cycle counts in the first wavefront %s, over all %d columns %s" % (first, n.size, sorted(set(int(v) for v in n))))
    assert len(first) > 1, first
