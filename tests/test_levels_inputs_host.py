"""The builders of tests/levels_common.py give inputs on which the kernels they feed can go wrong: asserted here on the C oracle and in
numpy alone, no device.  An input that went vacuous (no rain, one sub-cycle count per wavefront, one side of a branch only, W == 0,
state == reference state) fails here, before a GPU test passes for the wrong reason."""
import numpy as np
import pytest
import golden_util as gu
import levels_common as lc


def _finite(states, tracers=None):
    ok = all(np.isfinite(n[:, 1:-1, 1:-1]).all() and np.isfinite(e[:, 1:-1, 1:-1]).all() for n, e in states)
    return ok and (tracers is None or all(np.isfinite(t[:, 1:-1, 1:-1]).all() for t in tracers))


@pytest.mark.parametrize("L", lc.KESSLER_LEVELS)
def test_moist_supercell_rains_and_splits_the_rain_loop_unevenly(L):
    """moist_supercell on (ne3, 6 patches: 864 stored columns) at every level count the GPU test uses: after two consecutive oracle
    calls everything is finite and it has rained; the estimated sub-cycle count of the rain loop is 1 everywhere at dt = 5 s and, at
    dt = 400 s, takes at least two values inside one group of 64 consecutive stored columns (the lanes of one wavefront leave the loop
    at different times).  L = 3 is the one exception, stated: two level pairs of 6.7 km each never bind the CFL limit at 400 s, every
    column makes one pass there; the same conditions are therefore asserted, and the GPU test run, at levels_common.KESSLER_DT_L3 =
    800 s as well, where the counts are {1, 2} with 49 % of the columns above 1."""
    from oracle_lib import Oracle
    g, st, tr = lc.moist_supercell(3, L, seed=L)
    assert len(lc.stored_columns(g)) == 864
    # the draws as specified: vapour up to 3 % at the ground, cloud up to 3 g/kg, rain up to 2 % -- and next to nothing in other columns
    q = np.stack([t[:, 1:-1, 1:-1] / s[0][4][1:-1, 1:-1] for t, s in zip(tr, st)], 1)      # [3][patch][i][j][k]
    assert 0.027 < q[0, ..., 0].max() <= 0.03 and 2.7e-3 < q[1].max() <= 3e-3 and 0.015 < q[2].max() <= 0.02 and q.min() >= 0.0
    assert q[2].max(axis=-1).min() < 1e-3 * q[2].max()
    zl = [P.geom["z_levels"] for P in g.patches]
    for dt in (5.0, 400.0) + ((lc.KESSLER_DT_L3,) if L == 3 else ()):
        o = Oracle(g, fully_explicit=True, uniform_diffusion=(1500.0, 500.0))
        o.set_state(0, st); o.set_tracers(0, tr)
        pr = [np.zeros((P.na, P.nb)) for P in g.patches]
        o.kessler(0, dt, zl, pr); o.kessler(0, dt, zl, pr)
        assert _finite(o.get_state(0), o.get_tracers(0)), (L, dt)
        assert max(float(p[1:-1, 1:-1].max()) for p in pr) > 0.0, (L, dt)
        assert 1e-3 < max(gu.prognostic_errors(o.get_state(0), st)) < float("inf"), (L, dt)      # the call did something to the state
        n = lc.kessler_subcycles(g, st, tr, dt)
        distinct = max(len(set(n[i:i + 64].tolist())) for i in range(0, len(n) - 63, 64))
        print("L %d dt %g: sub-cycle counts %d..%d, %.0f %% of the columns above 1, up to %d distinct in a group of 64" % (L, dt, n.min(), n.max(), 100.0 * np.mean(n > 1), distinct))
        if dt == 5.0:
            assert n.min() == 1 and n.max() == 1, (L, sorted(set(n.tolist())))
        elif L >= 5 or dt == lc.KESSLER_DT_L3:
            assert distinct >= 2, (L, sorted(set(n.tolist())))
        else:
            assert n.max() == 1, (L, sorted(set(n.tolist())))


@pytest.mark.parametrize("L", lc.HELD_SUAREZ_LEVELS)
def test_held_suarez_case_reaches_both_sides_of_its_branches(L):
    """held_suarez_case: with the pinned surface pressure and L >= 5 the heating loop's sigma lies above 0.7 at some level and below it
    at another (max(0, (sigma - 0.7) / 0.3) takes both sides) and the equilibrium temperature is clamped to 200 K somewhere and left
    alone elsewhere.  L = 3 and 4 (lowest level at 5 km and 3.75 km of 30 km) cannot reach sigma > 0.7: they run the bs = 0 side only,
    with both sides of the clamp.  The friction loop's sigma (pressure from rho * rho*theta, as the reference states it) passes 0.7
    from L = 30 on, and so does the heating loop's with the tracked surface slots; W != 0 and the tracked slots are positive."""
    g, st, ps = lc.held_suarez_case(L)
    assert _finite(st)
    assert max(float(np.abs(e[3, 1:-1, 1:-1]).max()) for _, e in st) > 0.0
    assert all((e[[2, 4], 1:-1, 1:-1, 0] > 0.0).all() for _, e in st)
    assert all(np.all(np.abs(p / 1.0e5 - 1.0) <= 0.01) and np.ptp(p) > 1.0e3 for p in ps)
    sf, sh, teq = lc.held_suarez_branches(g, st, ps)
    sf_t, sh_t, _ = lc.held_suarez_branches(g, st, None)
    print("L %d: sigma heating %.3f..%.3f (tracked %.3f..%.3f), friction %.3f..%.3f, T_eq before the clamp %.1f..%.1f" % (
        L, sh.min(), sh.max(), sh_t.min(), sh_t.max(), sf.min(), sf.max(), teq.min(), teq.max()))
    assert teq.min() < 200.0 < teq.max()
    assert sh.min() < 0.7 and sf.min() < 0.7
    if L >= 5:
        assert sh.max() > 0.7
    else:
        assert sh.max() < 0.7 and sf.max() < 0.7 and sh_t.max() < 0.7
    if L >= 30:
        assert sf.max() > 0.7 and sh_t.max() > 0.7


@pytest.mark.parametrize("ne,L,npatch,case,ntr,dt", lc.INTERP_GRIDS, ids=lc.INTERP_IDS)
def test_interp_state_is_away_from_the_reference_state_and_w_is_not_zero(ne, L, npatch, case, ntr, dt):
    """interp_state: W != 0, every field differs from the reference state by more than 1e-3 of its size (so the comparisons without
    the reference state are not 0 / 0), the tracers are not zero; d_xi R differs between the nodes of an element by more than 1e-6
    relative, so dividing W by the first node's value can be told from dividing by each node's own -- on the Schar grid (4.5e-3),
    for which the grid is there, and on the two others as well (1.0e-2, 7.8e-3: it is not constant on the baroclinic-wave grids
    either)."""
    g, states = gu.make_grid(ne, L, npatch, case=case, ntracers=ntr)
    st, tr = lc.interp_state(g, states, dt=dt)
    assert _finite(st, tr)
    for c in range(5):
        loc = 1 if c == 3 else 0
        ref = "ref_redge" if c == 3 else "ref_node"
        big = max(float(np.abs(s[loc][c][1:-1, 1:-1]).max()) for s in st)
        far = max(float(np.abs(s[loc][c][1:-1, 1:-1] - np.asarray(P.geom[ref])[c][1:-1, 1:-1]).max()) for s, P in zip(st, g.patches))
        assert big > 0.0 and far > 1e-3 * big, (c, big, far)
    assert (tr is None) == (ntr == 0)
    if tr is not None:
        assert all(float(np.abs(t[c][1:-1, 1:-1]).max()) > 0.0 for t in tr for c in range(ntr))
    spread = 0.0
    for P in g.patches:
        d = np.asarray(P.geom["deriv_r_redge"])[..., 2]
        for a in range(1, P.na - 1, 4):
            for b in range(1, P.nb - 1, 4):
                spread = gu.worse(spread, float(np.max(np.abs(d[a:a + 4, b:b + 4] / d[a, b] - 1.0))))
    print("%s ne%d L%d: d_xi R differs by up to %.2e relative inside an element" % (case, ne, L, spread))
    assert spread > 1e-6


@pytest.mark.parametrize("npts,nreta", [(1, 1), (255, 4), (600, 4)])
def test_interp_points_rows_and_coefficients(npts, nreta):
    """interp_points: element-first nodes, coefficient rows that sum to one, exact 0 / 1 coefficients on the fixed first points, the
    operator rows as announced (top entry; dense; all zero; two adjacent weights), and the long-double restatement agrees with the C
    oracle to a few ulps of the field on them (the oracle's own distance, the yardstick of the device test)."""
    from oracle_lib import Oracle
    g, states = gu.make_grid(3, 5, 6, ntracers=2)
    pts = lc.interp_points(g, npts, nreta, seed=npts)
    L = g.L
    assert pts["patch"].min() >= 0 and pts["patch"].max() < 6 and (npts < 100 or len(set(pts["patch"].tolist())) == 6)
    assert np.all((pts["node_a"] - 1) % 4 == 0) and np.all((pts["node_b"] - 1) % 4 == 0) and pts["node_a"].max() <= 9 and pts["node_a"].min() >= 1
    assert np.allclose(pts["coeff_a"].sum(1), 1.0, atol=1e-14) and np.allclose(pts["coeff_b"].sum(1), 1.0, atol=1e-14)
    assert sorted(pts["coeff_a"][0].tolist()) == [0.0, 0.0, 0.0, 1.0] and sorted(pts["coeff_b"][0].tolist()) == [0.0, 0.0, 0.0, 1.0]
    if npts > 3:
        assert sorted(pts["coeff_a"][3].tolist()) == [0.0, 0.0, 0.0, 1.0] and pts["coeff_a"][3][1] == 1.0
        assert np.count_nonzero(pts["coeff_a"][2]) == 4
    opn, ope = pts["op_levels"], pts["op_interfaces"]
    assert opn.shape == (nreta, L) and ope.shape == (nreta, L + 1)
    assert np.count_nonzero(opn[0]) == 1 and opn[0, L - 1] == 1.0 and np.count_nonzero(ope[0]) == 1 and ope[0, L] == 1.0
    if nreta == 4:
        assert np.all(opn[1] != 0.0) and np.all(ope[1] != 0.0)
        assert not opn[2].any() and not ope[2].any()
        for op in (opn, ope):
            nz = np.nonzero(op[3])[0]
            assert len(nz) == 2 and nz[1] == nz[0] + 1 and abs(op[3].sum() - 1.0) < 1e-15
    st, tr = lc.interp_state(g, states)
    o = Oracle(g); o.set_state(0, st); o.set_tracers(0, tr)
    for inc in (True, False):
        for prim in (True, False):
            full, _ = lc.interp_longdouble(g, st, None, pts, 0, True, prim)
            want, twant = lc.interp_longdouble(g, st, tr, pts, 0, inc, prim)
            got = o.interpolate_state(0, pts, 0, inc, prim)
            dist = lc.field_distance(got, want, full)
            print("npts %d nreta %d reference state %s primitive %s: oracle vs long double per field" % (npts, nreta, inc, prim), ["%.1e" % v for v in dist])
            assert max(dist) < 16 * np.finfo(np.float64).eps, (inc, prim, dist)
    tdist = lc.field_distance(o.interpolate_tracers(0, pts), twant, twant)
    assert max(tdist) < 16 * np.finfo(np.float64).eps, tdist
