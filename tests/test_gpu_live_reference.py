"""The device against the REAL reference run live on the same host (oracle/_ref travels with the snapshot): BASELINE configs at full or reduced size, bit for bit; the two band-LU flavours.  A missing oracle/_ref fails these tests on a GPU host (golden_util.need_live_reference, TMX_REQUIRE_LIVE_REF)."""
import os
import numpy as np
import pytest
import golden_util as gu
from parity_common import EXACT, TOL_CALL, TOL_STEPS, _cmp, UDIFF, _supercell_case, _rank_engines_step, INFO_EARLY_TILES, INFO_LATE_TILES      # noqa: F401

pytestmark = pytest.mark.gpu


def test_hundred_steps_ne15_L30():
    """North-star gate at BASELINE config 2 (ne15 np4 L30, dt 300 s): fp64 state difference < 1e-10 after 100 ARS343
    steps, every variable.  Where the real reference binary travelled with the snapshot (oracle/_ref/tmx_ref_dump,
    built in the build container) it runs here, on the GPU box's host, and hands over ITS OWN inputs (geometry,
    operators, halo transforms, state after 2 steps): the device then reproduces the reference's state after 100
    further steps bit for bit.  Without the binary the run is checked against the C oracle on the synthesised grid."""
    import os, subprocess, tempfile
    import tmxd
    from tempestmodel_amd.engine import Engine
    from oracle_lib import Oracle
    ne, L, dt = 15, 30, 300.0
    # the reference with the netlib LAPACK of OpenBLAS: its band LU is evaluated with FMA kernels on every host, whereas
    # MKL 2021.4 takes a non-FMA level-2 path on the AMD host of the GPU box (tools/host_lapack_probe.sh; on the Intel
    # build host the two builds are bit-identical, tests/golden/lapack_spread.json)
    ref_bin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "tmx_ref_dump_lapack2")
    ref_end = None
    if os.path.exists(ref_bin):
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "ref.tmxd")
            env = dict(os.environ, MKL_THREADING_LAYER="SEQUENTIAL", OMP_NUM_THREADS="1")
            subprocess.run([ref_bin, "--mode", "steps", "--ne", str(ne), "--levels", str(L), "--dt", str(dt), "--warm", "2",
                            "--steps", "100", "--every", "100", "--geom", "1", "--out", out], env=env, check=True,
                           stdout=subprocess.DEVNULL, timeout=1500)
            rd = tmxd.read(out)
        g, _ = gu.grid_from_fixture(rd, override=True)
        start = gu.full_states(rd, "warm", 6)
        ref_end = gu.full_states(rd, "step100", 6)
        del rd
    else:
        g, states = gu.make_grid(ne, L, 6)
        o0 = Oracle(g); o0.set_state(0, states)
        for _ in range(2):
            assert o0.step_ars343(dt) == 0
        start = o0.get_state(0)
    o = Oracle(g); o.set_state(0, start)
    e = Engine(g); e.upload_state(0, start)
    try:
        for _ in range(100):
            e.step_ars343(dt)
        e.sync()
        got = e.download_state(0)
        for _ in range(100):
            assert o.step_ars343(dt) == 0
        errs_o = gu.prognostic_errors(got, o.get_state(0))
        print("ne15 L30, 100 steps vs C oracle:", errs_o)
        assert max(errs_o) <= EXACT, errs_o
        if ref_end is not None:
            errs_r = gu.prognostic_errors(got, ref_end)
            print("ne15 L30, 100 steps vs real reference (its own inputs):", errs_r)
            assert max(errs_r) < TOL_STEPS, errs_r          # the gate
            assert max(errs_r) <= EXACT, errs_r               # and in fact bit for bit
    finally:
        e.close()


def test_bench_workload_vs_live_reference():
    """The workload bench.py times (BASELINE config 3's grid: ne30 np4 L30, 24 patches, dt 150 s) at its FULL size against
    the real reference run live on the GPU box's host: the reference hands over its own geometry, operators, halo
    transforms and its state after 2 steps; three ARS343 steps later the device state equals the reference's bit for bit.
    Needs oracle/_ref (built in the build container; it travels with the snapshot)."""
    import os, subprocess, tempfile
    import tmxd
    from tempestmodel_amd.engine import Engine
    ref_bin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "tmx_ref_dump_lapack2")
    gu.need_live_reference(ref_bin)
    ne, L, dt, npatch = 30, 30, 150.0, 24
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "ref.tmxd")
        env = dict(os.environ, MKL_THREADING_LAYER="SEQUENTIAL", OMP_NUM_THREADS="1")
        subprocess.run([ref_bin, "--mode", "steps", "--ne", str(ne), "--levels", str(L), "--dt", str(dt), "--patches", str(npatch),
                        "--warm", "2", "--steps", "3", "--every", "3", "--geom", "1", "--out", out], env=env, check=True,
                       stdout=subprocess.DEVNULL, timeout=1500)
        rd = tmxd.read(out)
    g, _ = gu.grid_from_fixture(rd, override=True)
    assert len(g.patches) == npatch
    start = gu.full_states(rd, "warm", npatch)
    ref_end = gu.full_states(rd, "step3", npatch)
    del rd
    e = Engine(g)
    try:
        e.upload_state(0, start)
        for _ in range(3):
            e.step_ars343(dt)
        e.sync()
        errs = gu.prognostic_errors(e.download_state(0), ref_end)
        print("ne30 L30 24 patches, 3 steps vs the live reference:", errs)
        assert max(errs) <= EXACT, errs
    finally:
        e.close()


LIVE_CASES = [
    # name, dump-driver arguments, synthesiser case, tracers, engine options, stepper, dt, steps
    ("jw_tracers_p24", ["--ne", "8", "--levels", "12", "--tracers", "2"], "jw", 2, {}, "ars343", 200.0, 3),
    ("jw_ark232_oddL_p24", ["--ne", "6", "--levels", "9", "--scheme", "ark232", "--tracers", "1"], "jw", 1, {}, "ark232", 200.0, 3),
    ("jw_ars443_p24", ["--ne", "10", "--levels", "16", "--scheme", "ars443"], "jw", 0, {}, "ars443", 150.0, 2),
    ("jw_ars232_visc2_p24", ["--ne", "6", "--levels", "10", "--scheme", "ars232", "--hypervis", "2"], "jw", 0,
     {"nu": (2.0e5, 2.0e5, 2.0e5), "hypervis_order": 2}, "ars232", 200.0, 3),
    ("smallplanet_udiff_p24", ["--ne", "6", "--levels", "8", "--planet", "120", "--udiff", "1500", "500", "--explicitvertical", "--tracers", "2"],
     "smallplanet", 2, {"fully_explicit": True, "uniform_diffusion": (1500.0, 500.0)}, "ars343", 1.0, 3),
    ("jw_p96", ["--ne", "8", "--levels", "6", "--patches", "96"], "jw", 0, {}, "ars343", 200.0, 2),
    ("jw_tracers_L60_p24", ["--ne", "4", "--levels", "60", "--tracers", "3"], "jw", 3, {}, "ars343", 200.0, 2),
    ("jw_ars232_tracers_oddL_p24", ["--ne", "6", "--levels", "7", "--scheme", "ars232", "--tracers", "2"], "jw", 2, {}, "ars232", 150.0, 2),
    # Schar mountain on the reduced-radius sphere: topography (terrain-following metric with non-zero slopes) and a Rayleigh layer
    ("schar_p24", ["--case", "schar", "--ne", "6", "--levels", "10"], "schar", 0, {}, "ars343", 0.5, 3),
    ("schar_ars222_p6", ["--case", "schar", "--ne", "4", "--levels", "8", "--patches", "6", "--scheme", "ars222"], "schar", 0, {}, "ars222", 0.5, 3),
]


@pytest.mark.parametrize("name,args,case,ntr,opts,scheme,dt,nsteps", LIVE_CASES, ids=[c[0] for c in LIVE_CASES])
def test_live_reference_sweep(name, args, case, ntr, opts, scheme, dt, nsteps):
    """Configurations no committed fixture holds, against the real reference run live on the GPU box's host (its own geometry,
    operators and halo transforms; state after 2 steps): sub-panel patch layouts (24 and 96 patches) with tracers, odd level
    counts, the other steppers, order-2 viscosity, the supercell dynamics.  Identical doubles after 2-3 further steps.
    Needs oracle/_ref."""
    import os, subprocess, tempfile
    import tmxd
    from tempestmodel_amd.engine import Engine
    ref_bin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "tmx_ref_dump_lapack2")
    gu.need_live_reference(ref_bin)
    npatch = int(args[args.index("--patches") + 1]) if "--patches" in args else 24
    full = list(args) + ([] if "--patches" in args else ["--patches", "24"])
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "ref.tmxd")
        env = dict(os.environ, MKL_THREADING_LAYER="SEQUENTIAL", OMP_NUM_THREADS="1")
        subprocess.run([ref_bin, "--mode", "steps", "--dt", str(dt), "--warm", "2", "--steps", str(nsteps), "--every", str(nsteps),
                        "--geom", "1", "--out", out] + full, env=env, check=True, stdout=subprocess.DEVNULL, timeout=1500)
        rd = tmxd.read(out)
    g, _ = gu.grid_from_fixture(rd, override=True, case=case, ntracers=ntr)
    assert len(g.patches) == npatch
    for P in g.patches:
        for nm in ("ref_node", "ref_redge", "ref_tracers"):
            if "p%d/%s" % (P.index, nm) in rd:
                P.geom[nm] = rd["p%d/%s" % (P.index, nm)]
    e = Engine(g, n_instances=10, **opts)
    try:
        e.upload_state(0, gu.full_states(rd, "warm", npatch))
        if ntr:
            e.upload_tracers(0, gu.full_tracers(rd, "warm", npatch))
        for _ in range(nsteps):
            e.step(scheme, dt)
        e.sync()
        errs = gu.prognostic_errors(e.download_state(0), gu.full_states(rd, "step%d" % nsteps, npatch))
        terr = gu.tracer_errors(e.download_tracers(0), gu.full_tracers(rd, "step%d" % nsteps, npatch)) if ntr else [0.0]
        print(name, "vs the live reference:", errs, terr)
        assert max(errs) <= EXACT and max(terr) <= EXACT, (errs, terr)
    finally:
        e.close()


def test_shallow_water_24_patches_vs_live_reference():
    """BASELINE config 1's case (Williamson test 2, the stock SWTest2) on 24 patches against the real reference run live on the
    GPU box's host, on the reference's own 2-D geometry: four Strang steps from the analytic initial state (the first with
    fFirstStep), state and carried instance equal the reference's bit for bit.  Needs oracle/_ref."""
    import os, subprocess, tempfile
    import tmxd
    from tempestmodel_amd.cubed_sphere import CubedSphereGrid
    from tempestmodel_amd.engine import Engine
    ref_bin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "tmx_ref_dump_lapack2")
    gu.need_live_reference(ref_bin)
    ne, npatch, dt, nsteps = 8, 24, 200.0, 4
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "ref.tmxd")
        env = dict(os.environ, MKL_THREADING_LAYER="SEQUENTIAL", OMP_NUM_THREADS="1")
        subprocess.run([ref_bin, "--mode", "steps", "--case", "sw2", "--scheme", "strang", "--ne", str(ne), "--patches", str(npatch), "--dt", str(dt),
                        "--steps", str(nsteps), "--every", str(nsteps), "--geom", "1", "--out", out], env=env, check=True,
                       stdout=subprocess.DEVNULL, timeout=600)
        rd = tmxd.read(out)
    from tempestmodel_amd.cubed_sphere import ShallowWaterTest2
    g = CubedSphereGrid(ne, 1, 1.0, ppd=2, shallow_water=True)
    g.evaluate_test_case(ShallowWaterTest2())          # geometry of the synthesiser, replaced by the reference's below
    for P in g.patches:
        for nm in list(P.geom):
            if "p%d/%s" % (P.index, nm) in rd and np.shape(P.geom[nm]) == rd["p%d/%s" % (P.index, nm)].shape:
                P.geom[nm] = rd["p%d/%s" % (P.index, nm)]
        P.delta_a = float(rd["p%d/element_delta_a" % P.index][0]); P.delta_b = float(rd["p%d/element_delta_b" % P.index][0])
    g.dx = rd["op/dx_basis_1d"]; g.stiff = rd["op/stiffness_1d"]
    gu.override_halo_transforms(g, rd)

    def full(tag):
        out = []
        for P in g.patches:
            n = np.zeros((5, P.na, P.nb, 1)); e_ = np.zeros((5, P.na, P.nb, 2))
            n[[0, 1, 2]] = rd["state/%s/p%d/node" % (tag, P.index)]
            out.append((n, e_))
        return out
    e = Engine(g, n_instances=5)
    try:
        e.upload_state(0, full("initial"))
        for n in range(nsteps):
            e.step("strang", dt, first=(n == 0))
        e.sync()
        for inst, tag in ((0, "step%d" % nsteps), (1, "step%d_carry" % nsteps)):
            errs = gu.prognostic_errors(e.download_state(inst), full(tag))[:3]
            print("shallow water ne8 24 patches, instance %d vs the live reference:" % inst, errs)
            assert max(errs) <= EXACT, errs
    finally:
        e.close()


def test_supercell_kessler_24_patches_vs_live_reference():
    """BASELINE config 4's case on 24 patches (ne4 np4 L40: the stock SupercellTest state from the Fortran initialiser,
    --explicitvertical, uniform diffusion, three tracers, KesslerPhysics::Perform after every step) against the real reference
    run live on the GPU box's host (about a minute of host time: the initialiser is slow): three steps from its state after one
    step, state and tracers bit for bit.  Needs oracle/_ref."""
    import os, subprocess, tempfile
    import tmxd
    from tempestmodel_amd.engine import Engine
    ref_bin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "tmx_ref_dump_lapack2")
    gu.need_live_reference(ref_bin)
    ne, L, npatch, dt, nsteps = 4, 40, 24, 0.5, 3
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "ref.tmxd")
        env = dict(os.environ, MKL_THREADING_LAYER="SEQUENTIAL", OMP_NUM_THREADS="1")
        subprocess.run([ref_bin, "--case", "supercell", "--explicitvertical", "--physics", "kessler", "--mode", "steps", "--ne", str(ne),
                        "--levels", str(L), "--dt", str(dt), "--patches", str(npatch), "--warm", "1", "--steps", str(nsteps),
                        "--every", str(nsteps), "--geom", "1", "--out", out], env=env, check=True, stdout=subprocess.DEVNULL, timeout=1500)
        rd = tmxd.read(out)
    g, _ = gu.grid_from_fixture(rd, override=True, case="supercell")
    for P in g.patches:
        for nm in ("ref_node", "ref_redge", "ref_tracers"):
            P.geom[nm] = rd["p%d/%s" % (P.index, nm)]
    e = Engine(g, fully_explicit=True, uniform_diffusion=(1500.0, 500.0), nu=(0.0, 0.0, 0.0))
    try:
        e.set_level_heights()
        e.upload_state(0, gu.full_states(rd, "warm", npatch)); e.upload_tracers(0, gu.full_tracers(rd, "warm", npatch))
        for _ in range(nsteps):
            e.step_ars343(dt)
            e.kessler(0, dt)
        e.sync()
        errs = gu.prognostic_errors(e.download_state(0), gu.full_states(rd, "step%d" % nsteps, npatch))
        terr = gu.tracer_errors(e.download_tracers(0), gu.full_tracers(rd, "step%d" % nsteps, npatch))
        print("supercell + Kessler ne4 L40 24 patches, %d steps vs the live reference:" % nsteps, errs, terr)
        assert max(errs) <= EXACT and max(terr) <= EXACT, (errs, terr)
    finally:
        e.close()


def test_held_suarez_L60_24_patches_vs_live_reference():
    """BASELINE config 5's shape on 24 patches (ne16 np4 L60: 1.5 M points) against the real reference run live on the GPU
    box's host: the stock HeldSuarezTest state after 2 steps with forcing, its own geometry; 3 further steps of dynamics +
    HeldSuarezPhysics::Perform on the device equal the reference's bit for bit (about 4.4 M evaluations each of the forcing's
    pow / exp / log on developed data).  Needs oracle/_ref."""
    import os, subprocess, tempfile
    import tmxd
    from tempestmodel_amd.engine import Engine
    ref_bin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "tmx_ref_dump_lapack2")
    gu.need_live_reference(ref_bin)
    ne, L, dt, npatch = 16, 60, 200.0, 24
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "ref.tmxd")
        env = dict(os.environ, MKL_THREADING_LAYER="SEQUENTIAL", OMP_NUM_THREADS="1")
        subprocess.run([ref_bin, "--case", "heldsuarez", "--physics", "hs", "--mode", "steps", "--ne", str(ne), "--levels", str(L),
                        "--dt", str(dt), "--patches", str(npatch), "--warm", "2", "--steps", "3", "--every", "3", "--geom", "1",
                        "--out", out], env=env, check=True, stdout=subprocess.DEVNULL, timeout=1500)
        rd = tmxd.read(out)
    g, _ = gu.grid_from_fixture(rd, override=True, case="heldsuarez")
    for P in g.patches:
        P.lat = rd["p%d/hs_latitude" % P.index]
    start = [(rd["state/warm/p%d/node" % p], rd["state/warm/p%d/redge" % p]) for p in range(npatch)]
    ref_end = gu.full_states(rd, "step3", npatch)
    del rd
    e = Engine(g)
    try:
        e.set_physics_inputs(None)
        e.upload_state(0, start)
        for _ in range(3):
            e.step_ars343(dt)
            e.held_suarez(0, dt)
        e.sync()
        errs = gu.prognostic_errors(e.download_state(0), ref_end)
        print("Held-Suarez ne16 L60 24 patches, 3 steps + forcing vs the live reference:", errs)
        assert max(errs) <= EXACT, errs
    finally:
        e.close()


def test_band_lu_without_fused_multiply_add_flavour():
    """A reference linked to a BLAS without fused multiply-adds (plain netlib, MKL on some AMD hosts) evaluates the band LU's
    updates as multiply + subtract; the oracle restates that with orc_set_lu_fma(0) and the product with its option "lu_fma" = 0
    (both flavours of the band LU are compiled into the one library since round 6; TMX_LU_FMA=0 is the variable the test plumbing turns
    into the option).  The column solve of that flavour equals the oracle's in that mode bit for bit -- and differs from the default
    flavour, so the switch is not a no-op.  The child process takes the variable; the same two flavours in ONE process:
    test_both_band_lu_flavours_in_one_process."""
    import subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import os, sys
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
        import numpy as np
        import golden_util as gu
        from oracle_lib import Oracle, lib
        from tempestmodel_amd.engine import Engine
        d = gu.load("steps_ne4_L6_p24.npz")
        g, _ = gu.make_grid(4, 6, 24)
        start = gu.expand_compact(d, "step2", g)
        res = {}
        for fma in (1, 0):
            lib().orc_set_lu_fma(fma)
            o = Oracle(g); o.set_state(1, start); o.set_state(2, start)
            assert o.v_step_implicit(1, 2, 87.0) == 0
            res[fma] = o.get_state(2)
        lib().orc_set_lu_fma(1)
        e = Engine(g)
        e.upload_state(1, start); e.copy_data(1, 2); e.v_step_implicit(1, 2, 87.0); e.sync()
        got = e.download_state(2)
        e.close()
        print("RESULT", max(gu.prognostic_errors(got, res[0])), max(gu.prognostic_errors(got, res[1])))
    """ % (root, root))
    env = dict(os.environ, TMX_LU_FMA="0")
    env.pop("TMX_LIBRARY", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
    assert r.returncode == 0 and line, r.stderr[-2000:]
    err_nofma, err_fma = (float(v) for v in line[0].split()[1:])
    print("multiply + subtract flavour vs oracle without / with fused multiply-adds:", err_nofma, err_fma)
    assert err_nofma <= EXACT and EXACT < err_fma < float("inf")      # (inf: a value that is not finite, which is no difference of flavours)


def test_both_band_lu_flavours_in_one_process():
    """Option "lu_fma" of ONE library, two engines side by side: each equals the oracle in its mode, bit for bit, for the column solve and
    for three whole ARS343 steps, and the two differ from one another."""
    from oracle_lib import Oracle, lib
    from tempestmodel_amd.engine import Engine
    d = gu.load("steps_ne4_L6_p24.npz")
    g, _ = gu.make_grid(4, 6, 24)
    start = gu.expand_compact(d, "step2", g)
    got = {}
    try:
        for fma in (1, 0):
            lib().orc_set_lu_fma(fma)
            o = Oracle(g); o.set_state(0, start); o.set_state(1, start); o.set_state(2, start)
            assert o.v_step_implicit(1, 2, 87.0) == 0
            e = Engine(g, options={"lu_fma": fma})
            try:
                assert e.get_option("lu_fma") == fma
                e.upload_state(0, start); e.upload_state(1, start); e.copy_data(1, 2); e.v_step_implicit(1, 2, 87.0); e.sync()
                assert max(gu.prognostic_errors(e.download_state(2), o.get_state(2))) <= EXACT, fma
                for _ in range(3):
                    assert o.step_ars343(200.0) == 0
                    e.step_ars343(200.0)
                e.sync()
                got[fma] = e.download_state(0)
                assert max(gu.prognostic_errors(got[fma], o.get_state(0))) <= EXACT, fma
            finally:
                e.close()
    finally:
        lib().orc_set_lu_fma(1)
    assert EXACT < max(gu.prognostic_errors(got[0], got[1])) < float("inf")


def test_nofma_flavour_vs_live_mkl_reference():
    """Pins the multiply + subtract flavour of the band LU (option "lu_fma" = 0) to a REAL reference:
    the MKL-linked oracle/_ref/tmx_ref_dump run live on this host.  MKL 2021.4 dispatches a non-FMA level-2 path on the AMD
    hosts of the GPU boxes (tools/host_lapack_probe.sh), which is the host class the flavour exists for.  Whether THIS host is
    one is measured, not assumed: the MKL build and the OpenBLAS-netlib build (FMA kernels on every host) of the reference
    run the same 100 steps at ne4 L10; identical checksums mean MKL uses FMAs here, the default flavour is the matching one
    (test_hundred_steps_ne15_L30 covers it) and this test skips, saying so.  Otherwise BASELINE config 2 (ne15 np4 L30,
    dt 300 s) runs 100 ARS343 steps in the MKL reference, which hands over its own geometry and its state after 2 steps, and
    the multiply + subtract flavour must reproduce the reference's final state bit for bit."""
    import subprocess, sys, tempfile, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mkl_bin = os.path.join(root, "oracle", "_ref", "tmx_ref_dump")
    ob_bin = os.path.join(root, "oracle", "_ref", "tmx_ref_dump_lapack2")
    gu.need_live_reference(mkl_bin, ob_bin)
    env = dict(os.environ, MKL_THREADING_LAYER="SEQUENTIAL", OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
    sums = []
    for b in (mkl_bin, ob_bin):
        out = subprocess.run([b, "--mode", "steps", "--ne", "4", "--levels", "10", "--dt", "200", "--warm", "2", "--steps", "100",
                              "--every", "100", "--geom", "0"], env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                             universal_newlines=True, timeout=900).stdout
        sums.append([l for l in out.splitlines() if "checksum step100" in l])
    cpu = next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "?")
    print("host CPU:", cpu, "| MKL reference == OpenBLAS-netlib reference after 100 steps at ne4 L10:", sums[0] == sums[1])
    assert sums[0] and sums[1], "the reference binaries printed no checksum"
    if sums[0] == sums[1]:
        pytest.skip("MKL evaluates the band LU with fused multiply-adds on this host (%s): the default flavour is the matching one "
                    "(test_hundred_steps_ne15_L30); the multiply + subtract flavour has no live reference here" % cpu)
    with tempfile.TemporaryDirectory() as td:
        ref = os.path.join(td, "ref.tmxd")
        subprocess.run([mkl_bin, "--mode", "steps", "--ne", "15", "--levels", "30", "--dt", "300", "--warm", "2", "--steps", "100",
                        "--every", "100", "--geom", "1", "--out", ref], env=env, check=True, stdout=subprocess.DEVNULL, timeout=1500)
        code = textwrap.dedent("""
            import os, sys
            sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
            import golden_util as gu, tmxd
            from tempestmodel_amd.engine import Engine, LIB_PATH
            rd = tmxd.read(%r)
            g, _ = gu.grid_from_fixture(rd, override=True)
            start = gu.full_states(rd, "warm", 6); end = gu.full_states(rd, "step100", 6)
            e = Engine(g); e.upload_state(0, start)
            for _ in range(100):
                e.step_ars343(300.0)
            e.sync()
            got = e.download_state(0); e.close()
            print("RESULT", " ".join("%%.3e" %% v for v in gu.prognostic_errors(got, end)))
        """ % (root, root, ref))
        res = {}
        for flavour, fma in (("nofma", "0"), ("default", "1")):
            cenv = dict(os.environ, TMX_LU_FMA=fma)
            cenv.pop("TMX_LIBRARY", None)
            r = subprocess.run([sys.executable, "-c", code], env=cenv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=900)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
            assert r.returncode == 0 and line, r.stderr[-2000:]
            res[flavour] = [float(v) for v in line[0].split()[1:]]
    print("ne15 L30, 100 steps against the live MKL reference: nofma flavour", res["nofma"], "default flavour", res["default"])
    # (the default flavour against THIS reference shows the reference's own LAPACK-to-LAPACK spread, 1.9e-10 in W after 100 steps
    #  on the EPYC hosts -- tests/golden/lapack_spread.json -- which is why the flavour exists; printed above, not asserted)
    assert max(res["nofma"]) <= EXACT, res               # the multiply + subtract flavour IS this host's reference, bit for bit
    assert EXACT < max(res["default"]) < float("inf"), res              # and the switch is not a no-op on such a host
