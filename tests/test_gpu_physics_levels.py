"""The column physics kernels (Kessler microphysics, Held-Suarez forcing) against the C oracle, bit for bit, across level counts.

The fixtures these kernels came with fix one shape each (Kessler: ne2, L = 40, 384 columns; Held-Suarez: L = 30 and 60); what the kernels
do with a level count depends on it in closed form (tmx_k_physics.hip), so every count at which something changes is run here on a grid
whose column count fills no whole number of workgroups (ne3, 6 patches: 864 stored columns = 13.5 x 64 = 3.375 x 256).  Inputs:
tests/levels_common.py, qualified on the CPU by tests/test_levels_inputs_host.py.  Oracle and device see identical inputs: EXACT."""
import numpy as np
import pytest
import golden_util as gu
import levels_common as lc
from parity_common import EXACT, UDIFF

pytestmark = pytest.mark.gpu

INFO_UNIQUE_INSTANCES, INFO_UNIQUE_CONVERSIONS, INFO_PHYSICS_KERNEL = 13, 14, 24      # tmx_info (include/tempest_mi355x.h)


@pytest.mark.parametrize("L", lc.KESSLER_LEVELS)
def test_kessler_kernels_vs_oracle(L):
    """Two consecutive tmx_physics_kessler calls on levels_common.moist_supercell, dt = 5 s (one pass of the rain loop everywhere) and
    dt = 400 s (up to 31 sub-cycles, up to 25 different counts inside one wavefront at L = 60; {1, 2} at L = 5; one pass at L = 3, which
    therefore also runs dt = 800 s, {1, 2}): state, tracers and precipitation are the oracle's doubles.  k_kessler_tile deals the levels out to kt = ceil(L / 5) wavefronts, wavefront
    ty owning levels ty, ty + kt, ... in at most 5 register slots:

        L = 3       the engine's minimum; kt = 1, two empty slots
        L = 5       one full wavefront
        L = 6       first ragged kt = 2: levels 0, 2, 4 and 1, 3, 5; the top level (one-sided dz) in slot 2 of wavefront 1, slots 3, 4 empty
        L = 31, 32  the two sides of the opt-in to more than 48 KB of dynamic LDS (L x 1536 + 512 bytes: 48 128 and 49 664)
        L = 37      kt = 8 with three empty slots
        L = 40      the shape the suite already had, every slot full -- on this grid
        L = 41      the first level count the dispatcher gives to k_kessler (one lane per column) unasked
        L = 60      config 5's count, column kernel

    864 columns leave the last workgroup of k_kessler_tile half filled (32 lanes repeat the last column and store nothing) and the
    last one of k_kessler with 96 of 256 lanes.  For L <= 40 the same calls with the option kessler_column = 1 give the same bits
    from both kernels, raw (halo included: neither kernel writes there).  tmx_info(TMX_INFO_PHYSICS_KERNEL) tells which Kessler
    kernel ran and is asserted after every pair of calls: k_kessler_tile with kt = ceil(L / 5) up to L = 40 (2 | kt << 4), k_kessler (1)
    at 41 and 60 and under kessler_column = 1.

    Shown to bite in a scratch build: with `if (k < L - 1)` -> `if (k < L)` in front of the sedimentation term of k_kessler_tile (the
    top level then takes the two-sided form with zeros from above; in bounds) every L <= 40 fails the comparison with the oracle at
    dt = 5 s (rho*theta off by 1e-4 .. 6e-4 relative, RhoQr by 4e-3 .. 3e-2), L = 41 and 60, which run k_kessler, pass."""
    from tempestmodel_amd.engine import Engine
    from oracle_lib import Oracle
    g, st, tr = lc.moist_supercell(3, L, seed=L)
    zl = [P.geom["z_levels"] for P in g.patches]
    engines = []
    try:
        for options in [{}] + ([{"kessler_column": 1}] if L <= 40 else []):
            e = Engine(g, fully_explicit=True, uniform_diffusion=UDIFF, nu=(0.0, 0.0, 0.0), options=options)
            engines.append(e)
            e.set_level_heights()
            assert e.get_option("kessler_column") == (1.0 if options else 0.0)
        for dt in (5.0, 400.0) + ((lc.KESSLER_DT_L3,) if L == 3 else ()):
            o = Oracle(g, fully_explicit=True, uniform_diffusion=UDIFF)
            o.set_state(0, st); o.set_tracers(0, tr)
            want_pr = [np.zeros((P.na, P.nb)) for P in g.patches]
            o.kessler(0, dt, zl, want_pr); o.kessler(0, dt, zl, want_pr)
            assert max(float(p[1:-1, 1:-1].max()) for p in want_pr) > 0.0
            out = []
            for e in engines:
                e.upload_state(0, st); e.upload_tracers(0, tr)
                e.kessler(0, dt); e.kessler(0, dt); e.sync()
                kt = {3: 1, 5: 1, 6: 2, 31: 7, 32: 7, 37: 8, 40: 8, 41: 0, 60: 0}[L]      # 0: the column kernel
                assert e.info(INFO_PHYSICS_KERNEL) == (1 if e.options or not kt else 2 | kt << 4), (L, e.options, e.info(INFO_PHYSICS_KERNEL))
                gs, gt, pr = e.download_state(0), e.download_tracers(0), e.download_precipitation(reset=True)
                errs, terrs = gu.prognostic_errors(gs, o.get_state(0)), gu.tracer_errors(gt, o.get_tracers(0))
                print("Kessler L %d dt %g %s: vs oracle %s %s" % (L, dt, e.options or "default", errs, terrs))
                assert max(errs) <= EXACT and max(terrs) <= EXACT, (L, dt, e.options, errs, terrs)
                for P in g.patches:
                    assert np.array_equal(pr[P.index][1:-1, 1:-1], want_pr[P.index][1:-1, 1:-1]), (L, dt, e.options, P.index)
                out.append((gs, gt, pr))
            if len(out) == 2:
                for p in range(6):
                    assert np.array_equal(out[0][0][p][0], out[1][0][p][0]) and np.array_equal(out[0][0][p][1][3], out[1][0][p][1][3]), (L, dt, p)
                    assert np.array_equal(out[0][1][p], out[1][1][p]) and np.array_equal(out[0][2][p], out[1][2][p]), (L, dt, p)
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("L", lc.HELD_SUAREZ_LEVELS)
def test_held_suarez_kernels_vs_oracle(L):
    """One tmx_physics_held_suarez call of 100 s on levels_common.held_suarez_case.  The kernel is launched as blocks of 4 levels;
    k_held_suarez<true> (instance node-unique in, element-major out) launches L + 1 rows, the extra row k == L only copying W: at
    L = 4 that row sits alone in a block, at L = 3 it shares one with the levels, at L = 5 and 61 the last block is ragged, at L = 30
    the level rows are.  L = 3 and 4 run the bs = 0 side of the sigma branch only (test_levels_inputs_host.py), L >= 5 both.

      (a) pinned surface pressure, 1e5 (1 + 0.01 U(-1,1)) per stored node;
      (b) the tracked surface slots (set_physics_inputs(None)); the two tracked interface entries come back with the state;
      (c) the instance as one ARS343 step leaves it on a tracer-free engine with closed-form metric: node-unique.  The pinned pressure
          differs between the copies of a seam node, so the forcing cannot stay node-unique and k_held_suarez<true> forces every stored
          copy with its own inputs: before the call the instance is one of info(UNIQUE_INSTANCES), after it it is not, at the cost
          of ONE conversion (the counters tests/test_gpu_unique_layout.py reads; they cannot tell this route from converting first,
          which also counts one: the route is read from tmx_physics_held_suarez, taken whenever the instance is node-unique, owns its
          slot and the inputs differ between copies).  All level counts bring (c) about.  Should the route stop being taken,
          nothing here fails and the L + 1-row launch goes unrun at L = 3 and 4: re-check by hand the conditions in
          tmx_physics_held_suarez (tmx_step.hip: `u.built && ... && u.form[instance] == 1 && e->imap[instance] == instance &&
          u.mixed_option`, then `!shared`): the layout built, the instance node-unique and owning its slot, mixed_option at its
          default 1, no other instance mapped onto this one.

    Each equals the oracle on identical inputs, EXACT.

    Shown to bite in a scratch build: with `k > (FROM_U ? L : L - 1)` -> `k >= (...)` in k_held_suarez, which drops the last row of
    the launch (in bounds), variant (a) fails at every L by assertion: rho*theta 9.8e-7 (L = 3) .. 2.4e-7 (L = 61) from the oracle."""
    from tempestmodel_amd.engine import Engine
    from oracle_lib import Oracle
    g, st, ps = lc.held_suarez_case(L)

    def oracle(pinned, steps):
        for P in g.patches:
            P.geom.pop("hs_surface_pressure", None)
            if pinned:
                P.geom["hs_surface_pressure"] = ps[P.index]
        try:
            o = Oracle(g); o.set_state(0, st)
            for _ in range(steps):
                assert o.step_ars343(100.0) == 0
            o.held_suarez(0, 100.0)
            return o.get_state(0)
        finally:
            for P in g.patches:
                P.geom.pop("hs_surface_pressure", None)

    for variant, pinned, steps in (("a", True, 0), ("b", False, 0), ("c", True, 1)):
        want = oracle(pinned, steps)
        assert 1e-6 < max(gu.prognostic_errors(want, st)) < float("inf")      # the forcing did something
        e = Engine(g, options={"unique_layout": 1 if variant == "c" else 0})
        try:
            e.set_physics_inputs(ps if pinned else None)
            e.upload_state(0, st)
            if variant == "c":
                e.step_ars343(100.0)
                n0, c0 = e.info(INFO_UNIQUE_INSTANCES), e.info(INFO_UNIQUE_CONVERSIONS)
                assert n0 > 0, (L, n0)
            e.held_suarez(0, 100.0)
            if variant == "c":
                assert (e.info(INFO_UNIQUE_INSTANCES), e.info(INFO_UNIQUE_CONVERSIONS)) == (n0 - 1, c0 + 1), (L, n0, c0, e.info(INFO_UNIQUE_INSTANCES), e.info(INFO_UNIQUE_CONVERSIONS))
            e.sync()
            got = e.download_state(0)
            errs = gu.prognostic_errors(got, want)
            print("Held-Suarez L %d (%s): vs oracle %s" % (L, variant, errs))
            assert max(errs) <= EXACT, (L, variant, errs)
            if variant == "b":
                for (gn, ge), (on, oe) in zip(got, want):
                    assert np.array_equal(ge[[2, 4], 1:-1, 1:-1, 0], oe[[2, 4], 1:-1, 1:-1, 0])
        finally:
            e.close()
