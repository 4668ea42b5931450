"""The explicit-stage walk (k_h_walk) and the hyperviscosity walk (k_hv_walk) against the C oracle at every segment count.

Both kernels are one wavefront walking a SEGMENT of a column with a sliding register window, and what can go wrong on its own sits at
a segment's ends (the clamped first window, the recomputed (u x zeta)_xi and xi_dot of a segment that does not start at the bottom, the
bottom boundary condition from levels 0 and 1, the rigid lid written by the last segment) or in its steady state (the prefetch of level
k + 1 before level k's arithmetic).  The segment count comes from tmxk_h_walk_segments, which on every grid a test can afford returns
the maximum, L / 2: segments of two or three levels, whatever L.  Production runs three segments of ten levels (ne30 L30) and ONE of
sixty (ne120 L60).  So here the count is FORCED through the options the production library accepts (h_walk = -n, hv_walk = -n) on the
grid of test_gpu_column_solve_levels.py (ne3, 6 patches: 54 elements = 13.5 tiles, the last tile with a padding element):

    L = 3       h_walk 1 (all the clamp leaves)
    L = 4       1, 2 (2 is the default)
    L = 7       1, 2 (levels 0-3, 3-7), 3 (2, 2, 3: an unequal last segment)
    L = 30      1, 2, 3 (2 and 3 are ne30's), 4 (7, 8, 7, 8), 7, 15
    L = 31      1, 3, 15 (odd: unequal everywhere)
    L = 60      1 (ne120's), 2

hv_walk (a walk over L + 1 levels) takes -1, -2, -3 and -((L + 1) / 2) on the same engines; once per L both ask for 64 segments and
tmx_info must report the clamp (L / 2, (L + 1) / 2: restated here, not read back); one engine per L runs the level-parallel kernels
(h_walk = 0, hv_walk = 0).  tmx_info(TMX_INFO_STAGE_KERNEL / TMX_INFO_HYPERVIS_KERNEL) says which kernel ran with how many segments, so
a count that was clamped, or a silent drop to the level-parallel kernels, fails.

Oracle and device see identical inputs: EXACT per call, == 0.0 over steps (the project's bars, parity_common)."""
import numpy as np
import pytest
import golden_util as gu
from parity_common import EXACT, UDIFF, _rank_engines_step, INFO_EARLY_TILES, INFO_LATE_TILES

pytestmark = pytest.mark.gpu

# tmx_info (include/tempest_mi355x.h)
INFO_METRIC_CLOSED_FORM, INFO_UNIQUE_INSTANCES, INFO_PREFIX_STAGES, INFO_STAGE_KERNEL, INFO_HYPERVIS_KERNEL = 6, 13, 17, 22, 23
# flag bits of TMX_INFO_STAGE_KERNEL (<< 16): own coefficient, copy-by-copy reads, prefix stored, node-unique, V.StepExplicit fused, uniform diffusion
PM, DM, EM, UQ, FV, UD = 1, 2, 4, 8, 16, 32

H_WALK = {3: [1], 4: [1, 2], 7: [1, 2, 3], 30: [1, 2, 3, 4, 7, 15], 31: [1, 3, 15], 60: [1, 2]}


def _stage(e):
    """(segments, terms, flags) of the last explicit-stage launch; None: the level-parallel kernels."""
    v = e.info(INFO_STAGE_KERNEL)
    assert v >= 0, v      # -1: nothing launched
    return None if v == 0 else (v & 255, (v >> 8) & 255, v >> 16)


def _cases(L):
    """(h_walk, hv_walk, segments of k_h_walk, segments of k_hv_walk) per engine pair: the h_walk list of the table with hv_walk = -1, -2, -3,
    -((L + 1) / 2) dealt out beside it (the longer list decides, the shorter one repeats), then 64 segments asked of both -- the clamp,
    restated: L / 2 and (L + 1) / 2 -- and the level-parallel kernels (0: what tmx_info must then report)."""
    hs = H_WALK[L]
    hvs = []
    for n in (1, 2, 3, (L + 1) // 2):
        if n not in hvs:
            hvs.append(n)
    out = []
    for i in range(max(len(hs), len(hvs))):
        n, m = hs[i % len(hs)], hvs[i % len(hvs)]
        assert n <= L // 2      # (the table asks for nothing the clamp would change)
        out.append((-n, -m, n, min(m, (L + 1) // 2)))
    out.append((-64, -64, L // 2, (L + 1) // 2))
    out.append((0, 0, 0, 0))
    return out


def _rough(smooth, L, seed=11):
    """The smooth state with rho and rho*theta scaled per node by uniform(0.5, 2), W on interfaces uniform(-30, 30), and U, V scaled and
    shifted per level by amounts of their own magnitude: every level differs from its neighbours in every windowed variable, so a value
    taken from the wrong level cannot cancel."""
    rng = np.random.default_rng(seed)
    fu, fv = rng.uniform(0.5, 2.0, L), rng.uniform(0.5, 2.0, L)
    su, sv = rng.uniform(-1.0, 1.0, L), rng.uniform(-1.0, 1.0, L)
    out = []
    for node, edge in smooth:
        node = node.copy(); edge = edge.copy()
        node[0] = node[0] * fu + su * np.abs(node[0]).mean()
        node[1] = node[1] * fv + sv * np.abs(node[1]).mean()
        node[2] *= rng.uniform(0.5, 2.0, node[2].shape)
        node[4] *= rng.uniform(0.5, 2.0, node[4].shape)
        edge[3] = rng.uniform(-30.0, 30.0, edge[3].shape)
        out.append((node, edge))
    return out


def _finite(states):
    return all(np.isfinite(n).all() and np.isfinite(e).all() for n, e in states)


def _errs(got, want):
    """golden_util.prognostic_errors under the name this file and test_gpu_tracer_column_shapes.py use: a value that is not finite in a
    compared slot, on either side, comes back as inf.  (The helper once took its maxima with max(m, x), which drops a NaN: a level that a
    walk never wrote and that held NaN compared as 0.0 -- seen with the hyperviscosity walk made to skip a level, DESIGN.md section 2 --
    and this wrapper carried the finiteness check that the helper now makes itself.)"""
    return gu.prognostic_errors(got, want)


def _terrs(got, want):
    """golden_util.tracer_errors, in the same way."""
    return gu.tracer_errors(got, want)


def _scrub(e, states, dt, tracers=None, step=None):
    """One step from ANOTHER state with another time step, before the steps that are compared: every instance and every internal buffer of
    the engine that a step writes then holds values that are not the expected ones, so a store that a walk leaves out does not find the
    right answer of an earlier, identical step in its place.  (It cannot reach what NO step writes: see DESIGN.md section 2 on the
    hyperviscosity walk made to skip a level.)"""
    e.upload_state(0, states)
    if tracers is not None:
        e.upload_tracers(0, tracers)
    (step or (lambda: e.step_ars343(dt)))()


@pytest.mark.parametrize("L", sorted(H_WALK), ids=["L%d" % L for L in sorted(H_WALK)])
def test_stage_and_hyperviscosity_walks_vs_oracle(L):
    """Every segment count of _cases(L): H.StepExplicit per call on the element-major layout (k_h_walk<0, .., UQ = false, FV = false>) on a
    rough and a smooth state, then two ARS343 steps and one Strang step from the smooth one on the default (node-unique) layout and
    element-major -- the first ARS343 step reads the uploaded instance copy by copy, the second stores and uses a prefix, the stages
    carry 0 to 7 terms with and without their own coefficient, so the instantiations ride along at every count -- all equal to the C
    oracle; tmx_info says that the walk ran with the segments asked for (or the level-parallel kernels where 0 was asked)."""
    from tempestmodel_amd.engine import Engine
    from oracle_lib import Oracle
    g, states = gu.make_grid(3, L, 6)
    o = Oracle(g); o.set_state(0, states)
    assert o.step_ars343(100.0) == 0
    smooth = o.get_state(0)
    inputs = {"rough": _rough(smooth, L), "smooth": smooth}
    want = {}
    for key, st in inputs.items():
        o.set_state(1, st); o.set_state(2, st)
        o.h_step_explicit(1, 2, 87.0)
        want[key] = o.get_state(2)
    o.set_state(0, smooth)
    for _ in range(2):
        assert o.step_ars343(100.0) == 0
    assert o.step("strang", 100.0, first=True) == 0
    want["steps"] = o.get_state(0)
    for key, st in want.items():
        assert _finite(st), key      # a comparison with NaN would be vacuous
    bad = []      # every comparison that missed: (L, h_walk, hv_walk), which, errors -- all of them are run, then asserted empty
    for h, hv, n, m in _cases(L):
        tag = (L, h, hv)
        # a: per call, element-major; b: whole steps on the same engine
        e = Engine(g, options={"unique_layout": 0, "h_walk": h, "hv_walk": hv})
        try:
            assert e.info(INFO_STAGE_KERNEL) == -1 and e.info(INFO_HYPERVIS_KERNEL) == -1, tag      # nothing launched yet
            assert e.info(INFO_METRIC_CLOSED_FORM) == 1, tag
            for key, st in inputs.items():
                e.upload_state(1, st)
                e.copy_data(1, 2)
                e.h_step_explicit(1, 2, 87.0)
                e.sync()
                assert _stage(e) == ((n, 0, 0) if n else None), (tag, key, _stage(e))      # n segments, a plain base, UQ and FV clear
                errs = _errs(e.download_state(2), want[key])
                print("L %d h_walk %d per call %s:" % (L, h, key), errs)
                if not max(errs) <= EXACT:
                    bad.append((tag, "per call, " + key, errs))
            _scrub(e, states, 37.0)
            e.upload_state(0, smooth)
            for _ in range(2):
                e.step_ars343(100.0)
            sk = _stage(e)
            assert (sk is None) if n == 0 else (sk is not None and sk[0] == n and not sk[2] & (UQ | UD)), (tag, sk)
            e.step("strang", 100.0, first=True)
            e.sync()
            assert e.info(INFO_UNIQUE_INSTANCES) == 0, tag
            assert e.info(INFO_HYPERVIS_KERNEL) == 0, tag      # the element-major layout has no hyperviscosity walk
            errs = _errs(e.download_state(0), want["steps"])
            print("L %d h_walk %d hv_walk %d steps, element-major:" % tag, errs)
            if not max(errs) == 0.0:
                bad.append((tag, "steps, element-major", errs))
        finally:
            e.close()
        # b: whole steps on the default layout
        e = Engine(g, options={"h_walk": h, "hv_walk": hv})
        try:
            _scrub(e, states, 37.0)
            prefix0 = e.info(INFO_PREFIX_STAGES)
            e.upload_state(0, smooth)
            for _ in range(2):
                e.step_ars343(100.0)
            assert e.info(INFO_UNIQUE_INSTANCES) > 0, tag
            sk = _stage(e)
            if n:
                assert sk is not None and sk[0] == n and sk[2] & (UQ | FV) == (UQ | FV) and not sk[2] & UD, (tag, sk)
                assert e.info(INFO_PREFIX_STAGES) >= prefix0 + 1, tag
            else:
                assert sk is None, (tag, sk)
            assert e.info(INFO_HYPERVIS_KERNEL) == m, (tag, e.info(INFO_HYPERVIS_KERNEL))
            e.step("strang", 100.0, first=True)
            e.sync()
            sk = _stage(e)
            print("L %d h_walk %d hv_walk %d: last stage of the Strang step:" % tag, sk)
            assert (sk is None) if n == 0 else (sk is not None and sk[0] == n and sk[2] & (UQ | FV | UD) == (UQ | FV)), (tag, sk)
            assert e.info(INFO_HYPERVIS_KERNEL) == m, (tag, e.info(INFO_HYPERVIS_KERNEL))
            errs = _errs(e.download_state(0), want["steps"])
            print("L %d h_walk %d hv_walk %d steps, node-unique:" % tag, errs)
            if not max(errs) == 0.0:
                bad.append((tag, "steps, node-unique", errs))
        finally:
            e.close()
    assert not bad, bad


@pytest.mark.parametrize("L", [7, 30], ids=["L7", "L30"])
def test_stage_walk_segments_with_a_tracer(L):
    """The same grid with one tracer (element-major: the node-unique layout serves tracer-free engines): two ARS343 steps with one and with
    three segments per column, state and tracer equal to the oracle's."""
    from tempestmodel_amd.engine import Engine
    from oracle_lib import Oracle
    g, states = gu.make_grid(3, L, 6, ntracers=1)
    tr0 = [g.initial_tracers[p] for p in range(6)]
    o = Oracle(g); o.set_state(0, states); o.set_tracers(0, tr0)
    assert o.step_ars343(100.0) == 0
    smooth, tr = o.get_state(0), o.get_tracers(0)
    for _ in range(2):
        assert o.step_ars343(100.0) == 0
    want_s, want_t = o.get_state(0), o.get_tracers(0)
    assert _finite(want_s) and all(np.isfinite(t).all() for t in want_t)
    for n in (1, 3):
        e = Engine(g, options={"unique_layout": 0, "h_walk": -n, "hv_walk": -n})
        try:
            _scrub(e, states, 37.0, tracers=tr0)
            e.upload_state(0, smooth); e.upload_tracers(0, tr)
            for _ in range(2):
                e.step_ars343(100.0)
            e.sync()
            sk = _stage(e)
            assert sk is not None and sk[0] == n and not sk[2] & (UQ | UD), (L, n, sk)
            errs = _errs(e.download_state(0), want_s)
            terrs = _terrs(e.download_tracers(0), want_t)
            print("L %d h_walk %d with a tracer:" % (L, -n), errs, terrs)
            assert max(errs) == 0.0 and max(terrs) == 0.0, (L, n, errs, terrs)
        finally:
            e.close()


def test_stage_walk_segments_uniform_diffusion_explicit_vertical():
    """L = 7, the supercell configuration's dynamics (uniform diffusion, fully explicit vertical mode, two tracers) set up as
    test_uniform_diffusion_explicit_vertical_percall / _steps are, with h_walk_udiff = 2: per call H.StepExplicit runs the walk that applies
    the horizontal diffusion (UD), whole steps the one with V.StepExplicit's U, V part behind it (FV + UD: the window reaches down to level
    k - 2).  One, two and three segments, call by call and over two ARS343 steps, against the oracle with those tests' bar: == 0.0."""
    from tempestmodel_amd.engine import Engine
    from oracle_lib import Oracle
    L = 7
    g, states = gu.make_grid(3, L, 6, case="smallplanet", ntracers=2)
    tr0 = [g.initial_tracers[p] for p in range(6)]
    sdt = 1.0 * gu.ARS343_GAMMA
    o = Oracle(g, fully_explicit=True, uniform_diffusion=UDIFF); o.set_state(0, states); o.set_tracers(0, tr0)
    assert o.step("ars343", 1.0, first=True) == 0
    warm, trw = o.get_state(0), o.get_tracers(0)      # W != 0, state off the reference state
    want = []
    o.copy_data(0, 1)
    o.h_step_explicit(0, 1, sdt); want.append(("h_explicit", o.get_state(1), o.get_tracers(1)))
    o.v_step_explicit(0, 1, sdt); want.append(("v_explicit", o.get_state(1), o.get_tracers(1)))
    o.apply_dss(1); want.append(("dss", o.get_state(1), o.get_tracers(1)))
    steps = []
    for _ in range(2):
        assert o.step("ars343", 1.0) == 0
        steps.append((o.get_state(0), o.get_tracers(0)))
    for _, s, t in want:
        assert _finite(s) and all(np.isfinite(x).all() for x in t)
    assert _finite(steps[-1][0])
    assert max(_errs(want[0][1], warm)) > 0.0      # the call did something
    for n in (1, 2, 3):
        e = Engine(g, fully_explicit=True, uniform_diffusion=UDIFF, options={"h_walk": -n, "h_walk_udiff": 2})
        try:
            _scrub(e, states, 0.5, tracers=tr0, step=lambda: e.step("ars343", 0.5, first=True))
            e.upload_state(0, warm); e.upload_tracers(0, trw)
            e.copy_data(0, 1)
            for k, (tag, ws, wt) in enumerate(want):
                if k == 0:
                    e.h_step_explicit(0, 1, sdt)
                elif k == 1:
                    e.v_step_explicit(0, 1, sdt)
                else:
                    e.apply_dss(1)
                e.sync()
                if k == 0:
                    sk = _stage(e)
                    assert sk is not None and sk[0] == n and sk[2] & UD and not sk[2] & (UQ | FV), (n, sk)
                errs = _errs(e.download_state(1), ws)
                terrs = _terrs(e.download_tracers(1), wt)
                print("udiff L 7 h_walk %d %s:" % (-n, tag), errs, terrs)
                assert max(errs) == 0.0 and max(terrs) == 0.0, (n, tag, errs, terrs)
            for k, (ws, wt) in enumerate(steps):
                e.step("ars343", 1.0)
                e.sync()
                sk = _stage(e)
                assert sk is not None and sk[0] == n and sk[2] & (FV | UD) == (FV | UD) and not sk[2] & UQ, (n, sk)
                errs = _errs(e.download_state(0), ws)
                terrs = _terrs(e.download_tracers(0), wt)
                print("udiff L 7 h_walk %d step %d:" % (-n, k + 1), errs, terrs)
                assert max(errs) == 0.0 and max(terrs) == 0.0, (n, k, errs, terrs)
        finally:
            e.close()


@pytest.mark.parametrize("h,hv", [(-1, -1), (-3, -4)])
def test_walks_over_a_tile_list_on_three_ranks(h, hv):
    """wg_tile / wg_grid with a tile list: three loopback rank engines on ne10, 7 levels, 24 patches (25 elements each), node-unique, run
    the boundary-first launches over p.quads -- every rank reports early AND late tiles, in the element-major plan (tmx_info) and in the
    node-unique thread order (the layout's own tables), which is what makes the stages split.  ne10 is the smallest grid of 24 patches on
    three ranks that does: on ne6 and ne8 (9 and 16 elements per patch) every tile holds a column another rank needs, no tile is late
    (counted on plan-only engines; 24 patches take an even ne).  Three ARS343 steps equal ONE oracle of the whole grid on every rank's
    patches."""
    import ctypes
    from tempestmodel_amd.engine import Engine
    from oracle_lib import Oracle
    L, n_ranks = 7, 3
    g, states = gu.make_grid(10, L, 24)
    o = Oracle(g); o.set_state(0, states)
    assert o.step_ars343(100.0) == 0
    smooth = o.get_state(0)
    for _ in range(3):
        assert o.step_ars343(100.0) == 0
    want = o.get_state(0)
    assert _finite(want)
    ranks = [Engine(g, rank=r, n_ranks=n_ranks, options={"unique_layout": 1, "h_walk": h, "hv_walk": hv}) for r in range(n_ranks)]
    try:
        for e in ranks:
            assert e.info(INFO_EARLY_TILES) > 0 and e.info(INFO_LATE_TILES) > 0, (e.rank, e.info(INFO_EARLY_TILES), e.info(INFO_LATE_TILES))
            sizes = np.zeros(13, dtype=np.int32)      # tmx_debug_unique_tables, table 0: .., [6] early, [7] late tiles of the thread order in use
            e.lib.tmx_debug_unique_tables.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
            assert e.lib.tmx_debug_unique_tables(e.h, int(e.get_option("unique_tile_shape")), 0, sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 13) == 13
            assert sizes[6] > 0 and sizes[7] > 0, (e.rank, sizes)
            e.upload_state(0, states)
        Engine.loopback_group(ranks)
        _rank_engines_step(ranks, lambda e, k: e.step_ars343(37.0), 1)      # (_scrub, on all ranks together: the step exchanges)
        for e in ranks:
            e.upload_state(0, smooth)
        _rank_engines_step(ranks, lambda e, k: e.step_ars343(100.0), 3)
        Engine.loopback_dissolve(ranks[0])
        for e in ranks:
            assert e.info(INFO_UNIQUE_INSTANCES) > 0, e.rank
            sk = _stage(e)
            assert sk is not None and sk[0] == min(-h, L // 2) and sk[2] & (UQ | FV) == (UQ | FV), (e.rank, sk)
            assert e.info(INFO_HYPERVIS_KERNEL) == min(-hv, (L + 1) // 2), (e.rank, e.info(INFO_HYPERVIS_KERNEL))
            got = e.download_state(0)
            errs = _errs([got[p] for p in e.local_patches], [want[p] for p in e.local_patches])
            print("three ranks h_walk %d hv_walk %d rank %d:" % (h, hv, e.rank), errs)
            assert max(errs) == 0.0, (e.rank, errs)
    finally:
        for e in ranks:
            e.close()
