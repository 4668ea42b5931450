"""Tracer transport and both positive-definite filters against the C oracle where they ACT: tracer fields of any sign, one to sixteen
tracers, the level counts at which the kernels take another path.

The rest of the suite gives the tracer kernels positive fields (one fixture with compact support aside), at most four tracers, and
never calls tmx_v_filter_negative_tracers.  Both filters compute r = total / nonneg and store (q > 0) ? q * r : 0; on positive data
r = 1 and `>=` in place of `>` changes nothing.  Here (tests/tracer_inputs_common.py, qualified without a device by
tests/test_tracer_inputs_host.py) every patch holds elements and columns of mixed sign with r in (0, 1), of net negative mass (r < 0:
positive entries come out negative), of nothing positive (r = -inf) and of zeros alone (r = 0 / 0): the device agrees with the
reference there only if the product 0 * r is never formed and the per-node comparison is `>`.

Kernels: k_h_tracers<UD, NT> (flux update + fused filter), k_hypervis_tracers in its three uses (Laplacian into the work instance,
fourth-order update + filter, second-order update + filter), k_v_filter_tracers (behind V.StepImplicit, in Strang's carry-over step and
through its own entry point), the tracer column walks in groups of three (5 tracers: 3 + 2; 16: 5 x 3 + 1), and the DSS / exchange
over 5 L + 1 + nt L slabs.

Grid ne3 / 6 patches (864 columns = 13.5 tiles of 64: the last tile is half empty), (levels, tracers):

    (3, 1)      the minimum: one block of four level rows with a dead fourth row (kc clamped), a lone tracer
    (4, 5)      one full block; 3 + 2
    (5, 4)      one live row in the second block; 3 + 1
    (7, 16)     the ABI's maximum tracer count
    (30, 3)     the headline's level count

Oracle and device see identical inputs: EXACT per call and over steps (parity_common; 0.0 on the project's hosts), through
golden_util's helpers, for which a value that is not finite is a miss.  Every engine first runs one step on other tracers with
another time step (_scrub of the stage-walk file).

Option tracer_lincomb_pass = 1 is not run: the production library refuses it (experiments flavour only; asserted in
test_abi_and_host_logic.py)."""
import numpy as np
import pytest
import golden_util as gu
import tracer_inputs_common as tc
from parity_common import EXACT, UDIFF, _rank_engines_step, INFO_EARLY_TILES, INFO_LATE_TILES
from test_gpu_stage_walk_segments import _errs, _terrs, _scrub

pytestmark = pytest.mark.gpu

IDS = ["L%d_nt%d" % s for s in tc.SHAPES]
INFO_UNIQUE_INSTANCES = 13


def _engine(g, **kw):
    from tempestmodel_amd.engine import Engine
    return Engine(g, n_instances=tc.NINST, **kw)


def _miss(bad, tag, got, want, tol=EXACT):
    """Compare (state, tracers) pairs (``tol``: EXACT per call, 0.0 over steps: the project's bars); a miss is recorded, all
    comparisons of a test run, then ``bad`` is asserted empty."""
    errs, terrs = _errs(got[0], want[0]), _terrs(got[1], want[1])
    print(tag, errs, terrs)
    if not (max(errs) <= tol and max(terrs) <= tol):
        bad.append((tag, errs, terrs))


def _get(e, ix):
    e.sync()
    return e.download_state(ix), e.download_tracers(ix)


def _interior(t):
    return t[:, 1:-1, 1:-1]


@pytest.mark.parametrize("L,nt", tc.SHAPES, ids=IDS)
def test_tracer_calls_vs_oracle(L, nt):
    """(a) Per call on a rough and on the smooth state: H.StepExplicit(0, 1), V.StepImplicit in place on a copy (L >= 4: at L = 3 the
    implicit branch has no reference, header of test_gpu_tracer_column_shapes.py), StepAfterSubCycle(0, 3, 4) -- update AND work
    instance --, and a linear combination of the results with a negative coefficient: state and tracers equal the oracle's; every call
    changed every tracer and the oracle's result holds exact zeros and negative values (a comparison of untouched or positive data
    would say nothing about the filters)."""
    g, st, rough, tr, other = tc.case(L, nt)
    e = _engine(g)
    bad = []
    try:
        assert e.info(INFO_UNIQUE_INSTANCES) == 0      # element-major: the node-unique layout serves tracer-free engines
        _scrub(e, st, 37.0, tracers=other)
        for which, state in (("rough", rough), ("smooth", st)):
            want = tc.want_percall(L, nt, which)
            e.upload_state(0, state); e.upload_tracers(0, tr)
            e.copy_data(0, 1); e.h_step_explicit(0, 1, tc.DT)
            e.copy_data(0, 2)
            if L >= 4:
                e.v_step_implicit(2, 2, tc.DT)
            e.h_step_after_subcycle(0, 3, 4, tc.DT)
            e.copy_data(0, 5); e.linear_combine_data(tc.COMBINE, 5)
            for ix in (1, 2, 3, 4, 5):
                got = _get(e, ix)
                _miss(bad, (L, nt, which, "instance", ix), got, want[ix])
                if ix != 4 and (ix != 2 or L >= 4):
                    assert min(_terrs(got[1], tr)) > 0.0, (which, ix)      # the call changed every tracer
                    z, n = tc.fractions(want[ix][1])
                    assert (z > 0.0 or ix == 5) and n > 0.0, (which, ix, z, n)
    finally:
        e.close()
    assert not bad, bad


@pytest.mark.parametrize("L,nt", tc.SHAPES, ids=IDS)
def test_fused_horizontal_filters_in_isolation(L, nt):
    """(b) dt = 0.0: H.StepExplicit leaves base - 0 * (1 / J) * (flux divergence) -- the divergence is finite, so the product is a zero
    and the subtraction returns the base's double -- followed by the fused filter; StepAfterSubCycle leaves the filter followed by
    the DSS.  On the CPU the oracle's dt = 0 call equals its exported filter bit for bit (test_tracer_inputs_host.py).  The device's
    H.StepExplicit equals the oracle's same call, the export applied to the input, and the numpy restatement; and class by class from
    the INPUT's masks: elements with nothing positive come out all +0.0, all-zero elements stay +0.0, everything else equals the
    restatement bit for bit.  StepAfterSubCycle(0, 3, 4, 0.0) equals the oracle's in both instances."""
    g, st, _, tr, other = tc.case(L, nt)
    want = tc.want_percall(L, nt, "smooth", 0.0)
    tin, tout, _ = tc.want_filters(L, nt, False)
    plain = tc.filter_h_numpy(g, tin)
    e = _engine(g)
    bad = []
    try:
        _scrub(e, st, 37.0, tracers=other)
        e.upload_state(0, st); e.upload_tracers(0, tr)
        e.copy_data(0, 1); e.h_step_explicit(0, 1, 0.0)
        e.h_step_after_subcycle(0, 3, 4, 0.0)
        got = _get(e, 1)
        _miss(bad, (L, nt, "H.StepExplicit, dt = 0, vs the oracle's call"), got, want[1])
        for name, ref in (("export", tout), ("restatement", plain)):
            terrs = _terrs(got[1], ref)
            print(L, nt, "H.StepExplicit, dt = 0, vs the", name, terrs)
            if not max(terrs) <= EXACT:
                bad.append((name, terrs))
        seen = {"all <= 0": 0, "all zero": 0, "has positive": 0}
        for P, a, b, c in zip(g.patches, tin, got[1], plain):
            cin, cout, cpl = tc.cells(a, False), tc.cells(b, False), tc.cells(c, False)
            m = tc.class_masks(cin)
            for k in ("all <= 0", "all zero"):
                assert (cout[m[k]] == 0.0).all() and not np.signbit(cout[m[k]]).any(), (P.index, k)
            assert not np.signbit(cout[cout == 0.0]).any(), P.index
            if EXACT == 0.0:
                assert np.array_equal(cout[m["has positive"]], cpl[m["has positive"]]), P.index
            for k in seen:
                seen[k] += int(m[k].sum())
        print(L, nt, "elements by class:", seen)
        assert seen["has positive"] > 0 and (nt == 1 or (seen["all <= 0"] > 0 and seen["all zero"] > 0)), seen      # (3, 1): kind 0 alone
        for ix in (3, 4):
            _miss(bad, (L, nt, "StepAfterSubCycle, dt = 0, instance", ix), _get(e, ix), want[ix])
        assert max(_terrs(_get(e, 3)[1], tr)) > 0.0      # the filter acted
    finally:
        e.close()
    assert not bad, bad


@pytest.mark.parametrize("L,nt", tc.SHAPES, ids=IDS)
def test_vertical_filter_entry_point(L, nt):
    """(c) tmx_v_filter_negative_tracers on its own: upload, call, download.  The tracers equal the oracle's exported vertical filter and
    the numpy restatement; the -0.0 planted in a few entries, and every other zero, comes back as +0.0 (the reference stores = 0.0);
    the state of the instance and both neighbouring instances, tracers included, are unchanged.  (tmx_download_tracers fills interior
    nodes only, so the download shows no halo to compare.)"""
    g, st, rough, _, other = tc.case(L, nt)
    tin, tout, where = tc.want_filters(L, nt, True, plant=True)
    plain = tc.filter_v_numpy(g, tin)
    e = _engine(g)
    bad = []
    try:
        _scrub(e, st, 37.0, tracers=other)
        for ix in (1, 2, 3):
            e.upload_state(ix, rough if ix == 2 else st); e.upload_tracers(ix, tin if ix == 2 else other)
        e.v_filter_negative_tracers(2)
        got = _get(e, 2)
        for name, ref in (("export", tout), ("restatement", plain)):
            terrs = _terrs(got[1], ref)
            print(L, nt, "vertical filter vs the", name, terrs)
            if not max(terrs) <= EXACT:
                bad.append((name, terrs))
        assert max(_terrs(got[1], tin)) > 0.0      # it acted
        for a, b, ix in zip(got[1], tout, where):
            assert (a[tuple(ix)] == 0.0).all() and not np.signbit(a[tuple(ix)]).any()
            assert not np.signbit(_interior(a)[_interior(a) == 0.0]).any()
            if EXACT == 0.0:
                assert np.array_equal(_interior(a), _interior(b))
        assert max(_errs(got[0], rough)) == 0.0
        for ix in (1, 3):
            s, t = _get(e, ix)
            assert max(_errs(s, st)) == 0.0 and max(_terrs(t, other)) == 0.0, ix
            assert all(np.array_equal(_interior(a), _interior(b)) for a, b in zip(t, other)), ix
    finally:
        e.close()
    assert not bad, bad


def test_vertical_filter_without_tracers_is_a_no_op():
    """(c) On an engine without tracers the entry point returns OK and the instance is unchanged."""
    from tempestmodel_amd.engine import Engine
    g, st = gu.make_grid(3, 5, 6)
    e = Engine(g)
    try:
        e.upload_state(0, st)
        e.v_filter_negative_tracers(0)      # raises on a non-zero return
        e.sync()
        got = e.download_state(0)
        assert max(_errs(got, st)) == 0.0
        assert all(np.array_equal(a[0][[0, 1, 2, 4], 1:-1, 1:-1], b[0][[0, 1, 2, 4], 1:-1, 1:-1]) and np.array_equal(a[1][3, 1:-1, 1:-1], b[1][3, 1:-1, 1:-1])
                   for a, b in zip(got, st))
    finally:
        e.close()


@pytest.mark.parametrize("key", tc.VISC_KEYS)
def test_viscosity_orders_and_scaling_with_tracers(key):
    """(d) StepAfterSubCycle with tracers in the forms no other test runs, at (5, 4): second order (nu = 2e5: the state kernel is given
    (-dt, -nu_scalar), the tracer kernel (+dt, +nu_scalar) and the filter), order 0 and nu = 0 (a plain copy: no filter, no DSS),
    fourth order with reference_length = 0 (coefficients not scaled); and the Schar mountain (L = 6, two tracers) at orders 2 and 0,
    where the Rayleigh layer follows.  Per call on the rough state, then two ARS343 steps from the case's state, against the oracle."""
    (g, st, rough, tr, other), kw, dt = tc.visc_case(key)
    upd, work, steps = tc.want_visc(key)
    e = _engine(g, **kw)
    bad = []
    try:
        _scrub(e, st, 0.37 * dt, tracers=other)
        e.upload_state(0, rough); e.upload_tracers(0, tr)
        e.h_step_after_subcycle(0, 3, 4, dt)
        got = _get(e, 3)
        _miss(bad, (key, "StepAfterSubCycle, update instance"), got, upd)
        if key == "reflen0":      # fourth order with nu != 0: the work instance holds the first pass's Laplacians, DSS'ed
            _miss(bad, (key, "StepAfterSubCycle, work instance"), _get(e, 4), work)
        changed = max(_terrs(got[1], tr)) > 0.0
        assert changed == (key in ("order2", "reflen0", "schar_order2")), (key, changed)
        if key.startswith("schar_"):
            assert max(_errs(got[0], rough)) > 0.0, key      # the relaxation follows the copy
        e.upload_state(0, st); e.upload_tracers(0, tr)
        for k, want in enumerate(steps):
            e.step_ars343(dt)
            _miss(bad, (key, "ARS343 step", k + 1), _get(e, 0), want, tol=0.0)
    finally:
        e.close()
    assert not bad, bad


@pytest.mark.parametrize("L,nt", tc.SHAPES_UDIFF, ids=["L%d_nt%d" % s for s in tc.SHAPES_UDIFF])
def test_uniform_diffusion_fully_explicit_with_signed_tracers(L, nt):
    """(e) The small planet, fully explicit vertical mode, uniform diffusion (reference tracers 0.9 |t|): H.StepExplicit
    (k_h_tracers<true, *>), V.StepExplicit and StepImplicitTermsExplicitly per call on the rough state, then two ARS343 and two Strang
    steps, against the oracle."""
    g, st, rough, tr, other = tc.case(L, nt, name="smallplanet")
    calls, steps = tc.want_udiff(L, nt)
    e = _engine(g, fully_explicit=True, uniform_diffusion=UDIFF)
    bad = []
    try:
        _scrub(e, st, 0.5, tracers=other, step=lambda: e.step("ars343", 0.5, first=True))
        e.upload_state(0, rough); e.upload_tracers(0, tr)
        for ix, (name, want) in enumerate(calls, start=1):
            e.copy_data(0, ix)
            getattr(e, name)(0, ix, tc.DT_UDIFF)
            got = _get(e, ix)
            _miss(bad, (L, nt, name), got, want)
            assert min(_terrs(got[1], tr)) > 0.0, name
        e.upload_state(0, st); e.upload_tracers(0, tr)
        for scheme, first, want in steps:
            e.step(scheme, tc.DT_UDIFF, first=first)
            _miss(bad, (L, nt, scheme, "first" if first else "later"), _get(e, 0), want, tol=0.0)
    finally:
        e.close()
    assert not bad, bad


PROGRAMS = [(7, 4, "ars343"), (7, 4, "strang"), (7, 4, "ark232"), (7, 16, "ars343"), (7, 16, "strang")]


@pytest.mark.parametrize("L,nt,program", PROGRAMS, ids=["L%d_nt%d_%s" % p for p in PROGRAMS])
def test_whole_steps_with_signed_tracers(L, nt, program):
    """(f) Two steps of ARS343, of Strang (first = True, then first = False: the second step is LinearCombine + the vertical filter on
    its own) and of ARK232 with four and with sixteen tracers: state and tracers after each step equal the oracle's."""
    g, st, _, tr, other = tc.case(L, nt)
    want = tc.want_steps(L, nt, program)
    e = _engine(g)
    bad = []
    try:
        _scrub(e, st, 37.0, tracers=other)
        e.upload_state(0, st); e.upload_tracers(0, tr)
        for (scheme, first), w in zip(tc.STEP_PROGRAMS[program], want):
            e.step(scheme, tc.DT, first=first)
            _miss(bad, (L, nt, scheme, "first" if first else "later"), _get(e, 0), w, tol=0.0)
    finally:
        e.close()
    assert not bad, bad


@pytest.mark.parametrize("k", [0, 1], ids=["first_step", "second_step"])
def test_rank_engines_with_signed_tracers_vs_oracle(k):
    """(g) Three loopback rank engines on ne12 / 24 patches at (5, 4) -- the grid on which every rank owns early and late tiles
    (asserted, as test_multirank_production_steps_loopback does) --, the first and the second of two ARS343 steps, one case each
    (the second from the oracle's state after the first; the oracle advances one step per case): every rank's patches equal ONE
    oracle of the whole grid.  The tracer kernels then run over tile lists, on data that clips -- in the second step on tracers that
    the filters have already been through.  The first case also builds the ne12 grid, which is most of its time."""
    from tempestmodel_amd.engine import Engine
    L, nt = tc.SHAPE_RANKS
    g, st, _, tr, other = tc.case(L, nt, ne=12, npatch=24)
    want = tc.want_step(L, nt, "ars343", k, ne=12, npatch=24)
    start = (st, tr) if k == 0 else tc.want_step(L, nt, "ars343", 0, ne=12, npatch=24)
    n_ranks = 3
    ranks = [Engine(g, rank=r, n_ranks=n_ranks, n_instances=tc.NINST) for r in range(n_ranks)]
    try:
        assert all(e.info(INFO_EARLY_TILES) > 0 and e.info(INFO_LATE_TILES) > 0 for e in ranks)
        for e in ranks:
            e.upload_state(0, st); e.upload_tracers(0, other)
        Engine.loopback_group(ranks)
        _rank_engines_step(ranks, lambda e, i: e.step("ars343", 37.0, first=True), 1)      # (_scrub, on all ranks together: the step exchanges)
        for e in ranks:
            e.upload_state(0, start[0]); e.upload_tracers(0, start[1])
        _rank_engines_step(ranks, lambda e, i: e.step("ars343", tc.DT, first=(k == 0)), 1)
        Engine.loopback_dissolve(ranks[0])
        for e in ranks:
            gs, gt = e.download_state(0), e.download_tracers(0)
            lp = e.local_patches
            errs = _errs([gs[p] for p in lp], [want[0][p] for p in lp])
            terrs = _terrs([gt[p] for p in lp], [want[1][p] for p in lp])
            print("three ranks, step %d, rank %d:" % (k + 1, e.rank), errs, terrs)
            assert max(errs) == 0.0 and max(terrs) == 0.0, (e.rank, k, errs, terrs)
            assert min(_terrs([gt[p] for p in lp], [start[1][p] for p in lp])) > 0.0, (e.rank, k)      # the step changed every tracer
    finally:
        for e in ranks:
            e.close()
