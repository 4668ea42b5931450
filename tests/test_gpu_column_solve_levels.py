"""Every dispatch of the implicit column solve against the C oracle, bit for bit, across level counts.

tmxk_vi_fused picks its kernel at launch time from the number of unique columns (lane-group kernel / two-role pair kernel, one or two
pairs per workgroup, one or two assembly wavefronts) and from the level count (ring of three or two block rows by LDS occupancy); the
two-producer variant deals the L + 1 block rows of a column out by parity.  The grids small enough for committed fixtures never vary
the two together, so here every variant is FORCED on a tiny grid (ne3, 6 patches: 488 unique columns, 8 column groups of 64) through
options the production library accepts, at the level counts where something changes:

    L = 3       the minimum the engine accepts: 4 block rows, fewer than the two-producer ring (4 rows) holds
    L = 4       5 block rows: one more than that ring
    L = 7       odd L = an even number of block rows under two producers; one tracer
    L = 30      the headline's level count; two tracers
    L = 31      odd, production-sized
    L = 36, 37  the two sides of the automatic ring depth 3 -> 2 with two pairs per workgroup
    L = 48, 49  the two sides of the implicit tracer column kernel's shape switch (launch_vt_solve, tmx_k_tracer_solve.hip); two tracers
    L = 60      config 5's level count; two tracers

Above 60 levels only the variants a level count is there for run (NEW_VARIANTS; the thresholds are restated from the dispatcher's LDS sizes in
_auto_ring_depth / _expected_kernel and swept on the CPU by test_vertical_shapes_host.py), every engine after a step from another state (_scrub):

    L = 82, 83    two pairs per workgroup: the automatic ring depth returns from 2 to 3 (two workgroups no longer share a CU); 83 with two tracers
    L = 109, 110  one pair per workgroup: ring depth 3 -> 2
    L = 132, 133  one pair per workgroup: ring depth 2 -> 3
    L = 159, 160  the lane-group kernel keeps its solution in its ring of 16 block rows (480 doubles per column = 3 (L + 1) at L = 159): from 160
                  levels on the dispatcher hands the share to the pair kernel, whatever "vi_group" asks for (the group variant alone)
    L = 223       two pairs per workgroup: three ring rows no longer fit ONE workgroup (440 L + 66 000 bytes > 160 KB), two do up to L = 268;
                  two tracers

Oracle and device see identical inputs, so the bar is the project's own for that comparison: EXACT."""
import copy
import numpy as np
import pytest
import golden_util as gu
from parity_common import EXACT
from test_gpu_stage_walk_segments import _scrub

pytestmark = pytest.mark.gpu

INFO_UNIQUE_INSTANCES, INFO_COLUMN_KERNEL, INFO_COLUMN_VARIANT = 13, 20, 21      # tmx_info (include/tempest_mi355x.h)

LEVELS = [(3, 0), (4, 0), (7, 1), (30, 2), (31, 0), (36, 0), (37, 0), (48, 2), (49, 2), (60, 2)]
# above 60 levels: (L, tracers) and the variants run there
NEW_LEVELS = [(82, 0), (83, 2), (109, 0), (110, 0), (132, 0), (133, 0), (159, 0), (160, 0), (223, 2)]
NEW_VARIANTS = ("pair2_auto", "pair1", "pair1_2prod", "group")

_PAIR1 = {"vi_group": 0, "vi_pair_workgroup": 1, "vi_producers": 1}
_PAIR2 = {"vi_group": 0, "vi_pair_workgroup": 2}
VARIANTS = [
    ("group", {"vi_group": 1}),
    ("pair1", _PAIR1),
    ("pair1_2prod", {"vi_group": 0, "vi_pair_workgroup": 1, "vi_producers": 2}),
    ("pair2_auto", _PAIR2),                                           # ring depth chosen by the dispatcher
    ("pair2_ring2", dict(_PAIR2, vi_ring_depth=2)),
    ("pair2_ring3", dict(_PAIR2, vi_ring_depth=3)),
    ("pair2_cpw60", dict(_PAIR2, vi_columns_per_wavefront=60)),       # 9 groups: the last workgroup's second pair has no columns
    ("pair1_cpw37", {"vi_group": 0, "vi_pair_workgroup": 1, "vi_columns_per_wavefront": 37}),      # ragged last group
    ("pair1_stored", dict(_PAIR1, metric_stored=1)),                  # CLOSED = false instantiations
    ("pair2_stored", dict(_PAIR2, metric_stored=1)),
    # two producers need the closed-form metric: asked for on a stored-metric engine, the dispatcher must drop to one
    ("pair1_stored_2prod", {"vi_group": 0, "vi_pair_workgroup": 1, "vi_producers": 2, "metric_stored": 1}),
    ("group_nofma", {"vi_group": 1, "lu_fma": 0}),                    # band LU as multiply + subtract: oracle under orc_set_lu_fma(0)
    ("pair2_nofma", dict(_PAIR2, lu_fma=0)),
]


CU_LDS = 160 * 1024


def _pair_lds(L, pairs, depth):
    """Bytes of dynamic LDS of a workgroup of the pair kernel, restated from the dispatcher's LDS sizes (NOT read back from the engine)."""
    op_count, opw, rmtab, ring_nq, ftot = 10, 5, 512, 20, 3      # TMX_OP_COUNT, TMX_OPW, TMX_RMTAB_DOUBLES, TMX_RING_NQ, TMX_FTOT
    common = op_count * (L + 1) * opw * 8 + (2 * L + 1) * 8 + rmtab * 8      # operator tables, 1 - eta, exp / log tables
    return common + pairs * (depth * ring_nq * 64 * 8 + ftot * (L + 1) * 4 + 4 * 4)      # ring, fill-in masks, hand-over counters


def _auto_ring_depth(L, pairs):
    """The ring depth tmxk_vi_fused chooses on its own for one assembly wavefront per pair: three block rows, or two where two workgroups
    share a CU's 160 KB of LDS only with two -- or where three rows do not fit ONE workgroup."""
    if 2 * _pair_lds(L, pairs, 3) > CU_LDS and 2 * _pair_lds(L, pairs, 2) <= CU_LDS:
        return 2
    return 2 if _pair_lds(L, pairs, 3) > CU_LDS else 3


def test_auto_ring_depth_switches_between_36_and_37_levels():
    """The hand-derived range of the two-row ring with two pairs per workgroup (440 L + 66 000 bytes per workgroup with three rows,
    440 L + 45 520 with two, against half of 160 KB): L = 37 .. 82; one pair per workgroup keeps three rows up to L = 109
    (428 L + 35 252 bytes)."""
    assert [L for L in range(3, 200) if _auto_ring_depth(L, 2) == 2] == list(range(37, 83))
    assert [L for L in range(3, 200) if _auto_ring_depth(L, 1) == 2] == list(range(110, 133))
    # ... and where three rows do not fit one workgroup: from L = 223 on with two pairs (two rows fit up to 268), from 301 on with one (up to 324)
    assert [L for L in range(200, 269) if _auto_ring_depth(L, 2) == 2] == list(range(223, 269))
    assert [L for L in range(200, 325) if _auto_ring_depth(L, 1) == 2] == list(range(301, 325))
    assert _pair_lds(268, 2, 2) <= CU_LDS < _pair_lds(269, 2, 2) and _pair_lds(324, 1, 2) <= CU_LDS < _pair_lds(325, 1, 2)


def _expected_variant(name, L):
    """(pairs per workgroup, assembly wavefronts per pair, block rows of the ring) the dispatcher must have launched."""
    if name == "pair1_2prod":
        return (1, 2, 4)                          # two rows are being written at a time: the ring holds one more
    pairs = 2 if name.startswith("pair2") else 1
    depth = {"pair2_ring2": 2, "pair2_ring3": 3}.get(name, _auto_ring_depth(L, pairs))
    return (pairs, 1, depth)


def _group_serves(L):
    """The lane-group kernel writes the 3 (L + 1) entries of a column's solution into its ring of 16 block rows x 30 doubles."""
    return 3 * (L + 1) <= 16 * 30


def _check_kernel(e, name, L):
    """tmx_info after a launch: the kernel and the variant that really ran, whatever the options asked for."""
    kernel, variant = e.info(INFO_COLUMN_KERNEL), e.info(INFO_COLUMN_VARIANT)
    if name.startswith("group") and not _group_serves(L):
        # the pair kernel serves the share: 8 column groups of the closed-form metric = one pair per workgroup, two assembly wavefronts, ring of four
        assert _pair_lds(L, 1, 4) <= CU_LDS, L
        assert (kernel, variant & 15, (variant >> 4) & 15, variant >> 8) == (1, 1, 2, 4), (name, L, kernel, variant)
    elif name.startswith("group"):
        assert (kernel, variant) == (2, 0), (name, kernel, variant)
    else:
        assert kernel == 1 and variant > 0, (name, kernel, variant)      # a pair variant that fell back to the lane-group kernel fails here
        got = (variant & 15, (variant >> 4) & 15, variant >> 8)
        assert got == _expected_variant(name, L), (name, L, got)


def _finite(states, tracers):
    return all(np.isfinite(n).all() and np.isfinite(e).all() for n, e in states) and (tracers is None or all(np.isfinite(t).all() for t in tracers))


def _oracle_expectations(g, smooth, rough, tr, fma):
    """Per call on the rough and the smooth state, and two ARS343 steps + one Strang step from the smooth one, with the band LU
    rounded as `fma` says.  Every return code must be 0: a singular column would make the comparison vacuous."""
    from oracle_lib import Oracle, lib
    want = {}
    lib().orc_set_lu_fma(fma)
    try:
        o = Oracle(g)
        for key, st in (("rough", rough), ("smooth", smooth)):
            o.set_state(1, st); o.set_state(2, st)
            if tr is not None:
                o.set_tracers(1, tr); o.set_tracers(2, tr)
            assert o.v_step_implicit(1, 2, 87.0) == 0, (key, fma)
            want[key] = (o.get_state(2), o.get_tracers(2) if tr is not None else None)
        o.set_state(0, smooth)
        if tr is not None:
            o.set_tracers(0, tr)
        for _ in range(2):
            assert o.step_ars343(100.0) == 0, fma
        assert o.step("strang", 100.0, first=True) == 0, fma
        want["steps"] = (o.get_state(0), o.get_tracers(0) if tr is not None else None)
    finally:
        lib().orc_set_lu_fma(1)
    for key, (st, t) in want.items():
        assert _finite(st, t), (key, fma)
    return want


def _raw_equal(a, b):
    """The arrays as downloaded, duplicated seam nodes inside a patch included (the solve scatters its result to them)."""
    return all(np.array_equal(an[[0, 1, 2, 4]], bn[[0, 1, 2, 4]]) and np.array_equal(ae[3], be[3]) for (an, ae), (bn, be) in zip(a, b))


def _inputs(L, ntr):
    """(grid, its view without tracers, initial states, initial tracers or None, smooth state, its tracers or None, rough state)"""
    from oracle_lib import Oracle
    g, states = gu.make_grid(3, L, 6, ntracers=ntr)
    # the node-unique layout serves tracer-free engines only: a view of the same grid without its tracers (they are passive: the
    # state the oracle computes with them is the state without them, asserted below where ntr > 0)
    g0 = g
    if ntr:
        g0 = copy.copy(g); g0.ntracers = 0
    o = Oracle(g); o.set_state(0, states)
    if ntr:
        o.set_tracers(0, [g.initial_tracers[p] for p in range(6)])
    assert o.step_ars343(100.0) == 0
    smooth, tr = o.get_state(0), (o.get_tracers(0) if ntr else None)
    rng = np.random.default_rng(7)
    rough = []
    for node, edge in smooth:
        node = node.copy(); edge = edge.copy()
        node[2] *= rng.uniform(0.5, 2.0, node[2].shape)
        node[4] *= rng.uniform(0.5, 2.0, node[4].shape)
        edge[3] = rng.uniform(-30.0, 30.0, edge[3].shape)
        rough.append((node, edge))
    return g, g0, states, ([g.initial_tracers[p] for p in range(6)] if ntr else None), smooth, tr, rough


def _variants(L):
    if L <= 60:
        return VARIANTS
    names = ("group",) if L in (159, 160) else NEW_VARIANTS + (("pair2_nofma",) if L in (83, 223) else ())
    return [(n, o) for n, o in VARIANTS if n in names]


@pytest.mark.parametrize("L,ntr", LEVELS + NEW_LEVELS, ids=["L%d" % L for L, _ in LEVELS + NEW_LEVELS])
def test_column_solve_variants_vs_oracle(L, ntr):
    """Every variant of VARIANTS at L levels: V.StepImplicit per call on a rough state (lane-divergent pivots, asserted through the
    kernel's own statistics for the pair variants) and on a smooth one, then two ARS343 steps and one Strang step on the node-unique
    layout (the launch without a column table) and element-major -- all equal to the C oracle bit for bit, the tracers too; and
    tmx_info says that the variant asked for is the one that ran."""
    from tempestmodel_amd.engine import Engine
    g, g0, states, tr0, smooth, tr, rough = _inputs(L, ntr)
    want = {fma: _oracle_expectations(g, smooth, rough, tr, fma) for fma in sorted({int(o.get("lu_fma", 1)) for _, o in _variants(L)} | {1})}
    if ntr:
        for key in ("rough", "smooth", "steps"):
            assert max(gu.prognostic_errors(_oracle_expectations(g0, smooth, rough, None, 1)[key][0], want[1][key][0])) == 0.0, key
    first = {}
    scrub = L > 60      # (above 60 levels: every engine first takes a step from another state, with another time step)
    for name, options in _variants(L):
        fma = int(options.get("lu_fma", 1))
        pair = name.startswith("pair")
        closed = "metric_stored" not in options
        # 1, 2: per call on the element-major layout (column table and fill-in of the in-patch copies), rough and smooth
        e = Engine(g, options=options)
        try:
            assert e.info(INFO_COLUMN_KERNEL) == -1 and e.info(INFO_COLUMN_VARIANT) == -1, name      # nothing launched yet
            assert e.info(6) == (1 if closed else 0), name                                            # TMX_INFO_METRIC_CLOSED_FORM
            if scrub:
                _scrub(e, states, 37.0, tracers=tr0)
            for key, st in (("rough", rough), ("smooth", smooth)):
                e.upload_state(1, st)
                if ntr:
                    e.upload_tracers(1, tr)
                e.copy_data(1, 2)
                if pair and key == "rough":
                    e.pivot_stats(True)
                e.v_step_implicit(1, 2, 87.0)
                e.sync()
                if pair and key == "rough":
                    uni, tot = e.pivot_stats(False)
                    print("L %d %s: pivot steps on the wave-uniform path: %d of %d" % (L, name, uni, tot))
                    assert 0 < tot and uni < tot, (name, uni, tot)      # some steps did take the lane-divergent tails
                _check_kernel(e, name, L)
                got = e.download_state(2)
                errs = gu.prognostic_errors(got, want[fma][key][0])
                assert max(errs) <= EXACT, (name, key, errs)
                if ntr:
                    terrs = gu.tracer_errors(e.download_tracers(2), want[fma][key][1])
                    assert max(terrs) <= EXACT, (name, key, terrs)
                assert _raw_equal(got, first.setdefault((fma, key), got)), (name, key)
        finally:
            e.close()
        # 3: whole steps from the smooth start, on the default layout (node-unique where the engine is eligible: closed-form
        # metric, no tracers) and element-major with the tracers
        for unique in (True, False):
            e = Engine(g0 if unique else g, options=options if unique else dict(options, unique_layout=0))
            try:
                if scrub:
                    _scrub(e, states, 37.0, tracers=None if unique else tr0)
                e.upload_state(0, smooth)
                if ntr and not unique:
                    e.upload_tracers(0, tr)
                for _ in range(2):
                    e.step_ars343(100.0)
                if unique:      # the launch with a null column table ran (a stored-metric engine has no node-unique form)
                    assert (e.info(INFO_UNIQUE_INSTANCES) > 0) == closed, (name, e.info(INFO_UNIQUE_INSTANCES))
                else:
                    assert e.info(INFO_UNIQUE_INSTANCES) == 0, name
                e.step("strang", 100.0, first=True)
                e.sync()
                _check_kernel(e, name, L)
                errs = gu.prognostic_errors(e.download_state(0), want[fma]["steps"][0])
                assert max(errs) == 0.0, (name, unique, errs)
                if ntr and not unique:
                    terrs = gu.tracer_errors(e.download_tracers(0), want[fma]["steps"][1])
                    assert max(terrs) == 0.0, (name, unique, terrs)
            finally:
                e.close()
