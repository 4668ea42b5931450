"""The tracer column update (UpdateColumnTracers) against the C oracle at the shapes the other files leave open.

Every kernel of the family takes its right-hand side from one statement list (tmx_device.h: edge_sum, tracer_edge_flux, penalty_row,
tracer_rhs_row), and test_gpu_column_kernels.py holds the kernels to one another bit for bit -- with two tracers and six levels or
more.  What has an oracle on the other side elsewhere runs one to three tracers.  Open until here:

    four tracers    the column walk takes tracers in groups of three: a group of one behind a group of three
    one tracer      a lone group of one
    three levels    the engine's minimum: every four-node stencil is clipped at both ends at once, every level is a boundary level
                    or touches both

Grid: ne3, 6 patches, case smallplanet, the rough state and the tracer recipe of
test_column_walking_vertical_kernels_are_bit_identical_to_the_level_parallel_ones; (L, tracers) = (3, 4), (7, 4), (7, 1) -- seven levels
give ragged segments.  Oracle and device see identical inputs: EXACT (parity_common).

The implicit mode takes four levels where the explicit mode takes three.  The reference keeps the tracers' band matrix (kl = ku = 1: four
band rows with the fill-in row) in an L x L array, so at L = 3 its leading dimension is 3 and LAPACK's dgbtrf refuses it (info = -6, the
reference's "Triangulation failure").  The C oracle restates that storage and its own dgbsv does not check the leading dimension: at
L = 3 each column's sub-diagonal entry is the next column's fill-in entry, which the factorisation zeroes.  Measured at (3, 4): the
device's two kernels agree with one another and differ from the oracle by 1.27e-13 of the tracers' maximum in both calls -- and the
oracle with that array given four rows differs from itself by the same 1.27e-13, and not at all at L = 7.  Four levels are the fewest at
which the implicit branch has a reference; the explicit branch's matrix is the diagonal, which the three rows hold.

Above 60 levels (NEW_SHAPES, NEW_SHAPES_IMPLICIT) the launchers change their kernel shape with the level count; the shape that ran is read from
tmx_info and held against a restatement of the launchers' LDS formulas (_expected_vt, _expected_walks; swept on the CPU by
test_vertical_shapes_host.py), every engine after a step from another state (_scrub):

    implicit   70 | 71     the all-columns form with one row lane ("vt_rows" = 0): 32 -> 16 columns per workgroup
               141 | 142   16 columns no longer fit a CU: the row-lane kernel <32, 4> gives way to the one-lane form <1, 3>, the only launches of it
               284 | 285   the last level count 8 columns fit | both ABI calls refuse before they write
    explicit   79 | 80     "vt_column": 64 -> 32 columns per workgroup; 160: both ABI calls refuse before they write
               118         the walks' tables pass 48 KB of dynamic LDS
               146 | 147   the walk of the explicitly evaluated implicit terms (416 L + 4 504 bytes against 64 KB) -> level-parallel kernel
               156 | 157   the walks of the U,V penalty and of the tracers (416 L + 408 bytes) -> level-parallel / LDS-tiled kernel"""
import functools
import numpy as np
import pytest
import golden_util as gu
from parity_common import EXACT, UDIFF
from test_gpu_stage_walk_segments import _errs, _terrs, _finite, _scrub

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4), (7, 4), (7, 1)]
# (see above); 35 and 36 levels: the two sides of the one-row-lane kernel's switch from 64 to 32 columns per workgroup in the all-columns
# form -- its working set, (9L + 3) doubles per column, fits the 160 KB of a CU 64 times up to L = 35
SHAPES_IMPLICIT = [(4, 4), (7, 4), (7, 1), (35, 1), (36, 1)]
DT = 0.7
NEW_SHAPES = [(79, 1), (80, 1), (118, 1), (146, 1), (147, 1), (156, 1), (157, 1)]
NEW_SHAPES_IMPLICIT = [(70, 1), (71, 1), (141, 2), (142, 2), (284, 1)]
REFUSED_IMPLICIT, REFUSED_VT_COLUMN = (285, 1), (160, 1)
STEPS_NINST = 10            # data instances of the whole-step engines and oracles (ARK232 takes more than the default seven)
STEPS_SHAPE = (157, 0)      # whole steps above every walk threshold of the vertical kernels ((83, 2): test_gpu_column_solve_levels.py)
INFO_COLUMN_KERNEL, INFO_COLUMN_VARIANT, INFO_TRACER_COLUMN_KERNEL, INFO_VERTICAL_KERNELS = 20, 21, 25, 26      # tmx_info (include/tempest_mi355x.h)
CU_LDS = 160 * 1024
NTILES = 14      # ne3, 6 patches: 864 stored columns in 64-column tiles


def _expected_vt(L, rows, all_columns, lanes=16):
    """TMX_INFO_TRACER_COLUMN_KERNEL of launch_vt_solve, restated from its LDS formula ((9L + 3) doubles per column; NOT read back): row lanes |
    log2 columns << 8 | all columns << 16."""
    lds = lambda lw: (9 * L + 3) * lw * 8
    if rows and lds(16) <= CU_LDS:
        nr, lwb = (32, 4) if L > 48 else (16, 3)
    else:
        nr, lwb = 1, (6 if all_columns else {8: 3, 16: 4, 32: 5}.get(lanes, 6))
        while lwb > 3 and lds(1 << lwb) > CU_LDS:
            lwb -= 1
    assert lds(1 << lwb) <= CU_LDS, L      # (a test must not reach a shape that does not fit, except through a call that refuses)
    return nr | lwb << 8 | (1 if all_columns else 0) << 16


def _segments(option, ntiles, rows, target):
    """walk_segments (tmx_internal.h) restated: -n = n segments; -1000 = in pairs until the grid has `target` wavefronts, five rows each at least"""
    n = -option
    if option == -1000:
        n = 2
        while ntiles * n < target and rows // (n + 2) >= 5:
            n += 2
    return max(1, min(n, rows))


def _expected_walks(L, opts):
    """TMX_INFO_VERTICAL_KERNELS after V.StepExplicit and StepImplicitTermsExplicitly of the fully explicit mode, restated from the walks' LDS
    formulas (operator tables 10 x (L + 1) x 5, 1 - eta 2L + 1, the terms kernel's exp / log tables 512 doubles; 64 KB): 12 bits per kernel."""
    lds = lambda extra: (10 * (L + 1) * 5 + 2 * L + 1 + extra) * 8
    out = []
    for name, rows, target, extra in (("vx_walk", L, 4096, 0), ("vt_explicit_walk", L, 2048, 0), ("vite_walk", L + 1, 2048, 512)):
        w = opts.get(name, -1000)
        out.append(_segments(w, NTILES, rows, target) if w < 0 and lds(extra) <= 64 * 1024 else 0)
    if opts.get("vt_column"):
        lw = 64 if (4 * L + 2) * 64 * 8 <= CU_LDS else 32
        assert (4 * L + 2) * lw * 8 <= CU_LDS, L
        out[1] = 0x800 | lw
    return out[0] | out[1] << 12 | out[2] << 24


@functools.lru_cache(maxsize=None)
def _case(L, nt):
    """(grid, rough state, tracers); the reference columns of the uniform diffusion are the smooth state and 0.9 x the tracers."""
    g, st = gu.make_grid(3, L, 6, case="smallplanet", ntracers=nt)
    rng = np.random.default_rng(5)
    tr = [np.abs(1e-3 * node[4][None] * (1.0 + 0.1 * rng.standard_normal((nt,) + node[4].shape))) for node, _ in st]
    for P, (n, e_), t in zip(g.patches, st, tr):
        P.geom["ref_node"] = n.copy(); P.geom["ref_redge"] = e_.copy(); P.geom["ref_tracers"] = 0.9 * t
    # a rough state: the penalty terms and the diffusion stencils see sign changes and large gradients
    rough = []
    for n, e_ in st:
        n = n.copy(); e_ = e_.copy()
        n[0] += rng.uniform(-20.0, 20.0, n[0].shape); n[1] += rng.uniform(-20.0, 20.0, n[1].shape)
        n[2] *= 1.0 + 0.01 * rng.standard_normal(n[2].shape); n[4] *= 1.0 + 0.01 * rng.standard_normal(n[4].shape)
        e_[3] = rng.uniform(-3.0, 3.0, e_[3].shape)
        rough.append((n, e_))
    return g, rough, tr


def _oracle_calls(L, nt, calls, **mode):
    """What the oracle leaves in instances 1, 2 after calls[0](0, 1, DT), calls[1](0, 2, DT) on copies of instance 0: [(state, tracers)] * 2"""
    from oracle_lib import Oracle
    g, rough, tr = _case(L, nt)
    o = Oracle(g, **mode)
    o.set_state(0, rough); o.set_tracers(0, tr)
    want = []
    for ix, name in ((1, calls[0]), (2, calls[1])):
        o.copy_data(0, ix)
        r = getattr(o, name)(0, ix, DT)
        assert not r, (name, r)
        want.append((o.get_state(ix), o.get_tracers(ix)))
        assert _finite(want[-1][0]) and all(np.isfinite(t).all() for t in want[-1][1]), name      # a comparison with NaN would be vacuous
    assert max(_terrs(want[0][1], tr)) > 0.0      # the update changed the tracers
    return want


def _device_calls(e, L, nt, calls, scrub=False, info=None):
    """info: tmx_info codes read after each call, appended to the call's entry"""
    g, rough, tr = _case(L, nt)
    if scrub:      # a step from another state with another time step first (every buffer a call writes then holds other values)
        e.upload_state(0, [(P.geom["ref_node"], P.geom["ref_redge"]) for P in g.patches]); e.upload_tracers(0, [0.5 * t for t in tr])
        for ix in (1, 2):
            e.copy_data(0, ix)
            getattr(e, calls[ix - 1])(0, ix, 0.37)
    e.upload_state(0, rough); e.upload_tracers(0, tr)
    got = []
    for ix, name in ((1, calls[0]), (2, calls[1])):
        e.copy_data(0, ix)
        getattr(e, name)(0, ix, DT)
        e.sync()
        got.append((e.download_state(ix), e.download_tracers(ix)) + (tuple(e.info(k) for k in info) if info else ()))
    return got


def _compare(bad, tag, calls, got, want):
    for name, (gs, gt, *_), (ws, wt) in zip(calls, got, want):
        errs, terrs = _errs(gs, ws), _terrs(gt, wt)
        print(tag, name, errs, terrs)
        if not (max(errs) <= EXACT and max(terrs) <= EXACT):
            bad.append((tag, name, errs, terrs))


@pytest.mark.parametrize("ud", [True, False], ids=["udiff", "plain"])
@pytest.mark.parametrize("L,nt", SHAPES + NEW_SHAPES, ids=["L%d_nt%d" % s for s in SHAPES + NEW_SHAPES])
def test_explicit_tracer_column_update_vs_oracle(L, nt, ud):
    """Fully explicit vertical mode, with and without uniform diffusion: V.StepExplicit (U,V penalty and the tracer columns) and
    StepImplicitTermsExplicitly as column walks with the default segment count, 1, 2 and 64 (clamped to the rows there are) segments, as
    the level-parallel kernels (0), and the tracers by the one-lane-per-column kernel (vt_column): state and tracers equal the oracle's."""
    from tempestmodel_amd.engine import Engine
    g, _, tr = _case(L, nt)
    mode = dict(fully_explicit=True, uniform_diffusion=UDIFF if ud else None)
    calls = ("v_step_explicit", "v_step_implicit_terms_explicitly")
    want = _oracle_calls(L, nt, calls, **mode)
    bad = []
    variants = [{"vx_walk": w, "vite_walk": w, "vt_explicit_walk": w} for w in (-1000, -1, -2, -64, 0)] + [{"vt_column": 1}]
    for opts in variants:
        e = Engine(g, options=opts, **mode)
        try:
            assert e.info(INFO_VERTICAL_KERNELS) == -1, opts      # nothing launched yet
            got = _device_calls(e, L, nt, calls, scrub=(L, nt) in NEW_SHAPES, info=(INFO_VERTICAL_KERNELS,))
        finally:
            e.close()
        # the three kernels that ran, each as the walk with the predicted segment count or as its level-parallel form
        assert got[1][2] == _expected_walks(L, opts), (L, opts, hex(got[1][2]), hex(_expected_walks(L, opts)))
        assert max(_terrs(got[0][1], tr)) > 0.0, opts      # the update changed the tracers
        _compare(bad, (L, nt, ud, opts), calls, got, want)
    assert not bad, bad


@pytest.mark.parametrize("L,nt", SHAPES_IMPLICIT + NEW_SHAPES_IMPLICIT, ids=["L%d_nt%d" % s for s in SHAPES_IMPLICIT + NEW_SHAPES_IMPLICIT])
def test_implicit_tracer_column_update_vs_oracle(L, nt):
    """Implicit vertical mode: the tracer columns behind the column solve of V.StepImplicit (unique columns, dependents written along) and
    ARK232's all-columns form at the end of StepImplicitTermsExplicitly, by the row-lane kernel (vt_rows = 1, the default) and by its
    one-row-lane form (0: k_vi_tracers_rows<1, .>, the serial order): state and tracers equal the oracle's.
    The two are one kernel text: between them vt_rows = 0 cross-checks the row-lane decomposition (ownership of rows, barriers, the
    register-carried pivot row) against its own serial form.  The separately written factorisation is on the other side of this
    comparison: the oracle's orc_dgbsv, which the CPU tests pin against LAPACK."""
    from tempestmodel_amd.engine import Engine
    g, _, tr = _case(L, nt)
    calls = ("v_step_implicit", "v_step_implicit_terms_explicitly")
    want = _oracle_calls(L, nt, calls)
    assert max(_terrs(want[1][1], tr)) > 0.0
    bad = []
    for rows in (1, 0):
        e = Engine(g, options={"vt_rows": rows})
        try:
            assert e.info(INFO_TRACER_COLUMN_KERNEL) == -1, rows      # nothing launched yet
            got = _device_calls(e, L, nt, calls, scrub=(L, nt) in NEW_SHAPES_IMPLICIT, info=(INFO_TRACER_COLUMN_KERNEL,))
        finally:
            e.close()
        # the shape that ran: the unique columns behind V.StepImplicit, every stored column behind StepImplicitTermsExplicitly
        assert (got[0][2], got[1][2]) == (_expected_vt(L, rows, False), _expected_vt(L, rows, True)), (L, rows, got[0][2], got[1][2])
        assert max(_terrs(got[0][1], tr)) > 0.0 and max(_terrs(got[1][1], tr)) > 0.0, rows      # both updates changed the tracers
        _compare(bad, (L, nt, "vt_rows", rows), calls, got, want)
    assert not bad, bad


def test_the_shapes_predicted_at_the_new_level_counts():
    """The restated predictions say what the level counts are there for (no device call: the device tests hold tmx_info against them)."""
    code = lambda nr, lwb, all_: nr | lwb << 8 | all_ << 16
    assert _expected_vt(141, 1, False) == code(32, 4, 0) and _expected_vt(142, 1, False) == code(1, 3, 0) and _expected_vt(284, 1, False) == code(1, 3, 0)
    assert _expected_vt(70, 0, True) == code(1, 5, 1) and _expected_vt(71, 0, True) == code(1, 4, 1)
    assert _expected_vt(141, 1, True) == code(32, 4, 1) and _expected_vt(142, 0, True) == code(1, 3, 1)
    seg = lambda L, o: [(_expected_walks(L, o) >> s) & 0xfff for s in (0, 12, 24)]
    auto = {}
    assert all(n > 0 for L in (79, 80, 118, 146) for n in seg(L, auto))                  # three walks
    assert [n > 0 for n in seg(147, auto)] == [True, True, False] and [n > 0 for n in seg(156, auto)] == [True, True, False]      # one kernel of each kind
    assert seg(157, auto) == [0, 0, 0] and seg(157, {"vx_walk": -2, "vite_walk": -2, "vt_explicit_walk": -2}) == [0, 0, 0]      # a forced -2 too
    assert seg(156, {"vx_walk": -2, "vite_walk": -2, "vt_explicit_walk": -2}) == [2, 2, 0] and seg(146, {"vite_walk": -64})[2] == 64
    assert seg(79, {"vt_column": 1})[1] == 0x800 | 64 and seg(80, {"vt_column": 1})[1] == 0x800 | 32


def _refused(e, call, ix, *words):
    """The ABI call raises TMX_ERR_UNSUPPORTED with a message that names the kernel and the largest level count it serves"""
    from tempestmodel_amd.engine import TempestError
    with pytest.raises(TempestError) as ei:
        getattr(e, call)(0, ix, DT)
    print(call, "->", ei.value)
    assert ei.value.code == -2, ei.value      # TMX_ERR_UNSUPPORTED
    assert all(w in str(ei.value) for w in words), (str(ei.value), words)


@pytest.mark.parametrize("mode", ["implicit", "vt_column"])
def test_a_level_count_the_tracer_kernel_does_not_serve_is_refused_before_any_write(mode):
    """285 levels in the implicit mode (8 columns of k_vi_tracers_rows need (9L + 3) x 8 x 8 = 164 352 bytes) and 160 levels with "vt_column" in the
    fully explicit mode ((4L + 2) x 32 x 8 = 164 352 bytes): V.StepImplicit / V.StepExplicit and StepImplicitTermsExplicitly, and a whole step,
    return TMX_ERR_UNSUPPORTED naming the kernel and its limit BEFORE their first kernel -- the update instance and its tracers are bit for bit
    what was uploaded (the column solve, the terms kernel and the U,V penalty have not run).  Nothing is launched with an oversized request."""
    from tempestmodel_amd.engine import Engine
    implicit = mode == "implicit"
    L, nt = REFUSED_IMPLICIT if implicit else REFUSED_VT_COLUMN
    g, rough, tr = _case(L, nt)
    kw = {} if implicit else dict(fully_explicit=True)
    e = Engine(g, options={} if implicit else {"vt_column": 1}, **kw)
    try:
        e.upload_state(0, rough); e.upload_tracers(0, tr)
        marked = [(n * 1.25, ed * 0.75) for n, ed in rough]
        for ix in (1, 2):
            e.upload_state(ix, marked); e.upload_tracers(ix, [2.0 * t for t in tr])
        e.sync()
        before = {ix: (e.download_state(ix), e.download_tracers(ix)) for ix in (0, 1, 2)}
        kernel, limit = ("k_vi_tracers_rows", "284") if implicit else ("k_v_tracers_explicit_column", "159")
        _refused(e, "v_step_implicit" if implicit else "v_step_explicit", 1, kernel, "%d levels" % L, "up to %s levels" % limit)
        _refused(e, "v_step_implicit_terms_explicitly", 2, kernel, "%d levels" % L, "up to %s levels" % limit)
        from tempestmodel_amd.engine import TempestError
        with pytest.raises(TempestError) as ei:
            e.step_ars343(DT)
        assert kernel in str(ei.value) and limit in str(ei.value), str(ei.value)
        e.sync()
        assert e.info(INFO_COLUMN_KERNEL) == -1 and e.info(INFO_TRACER_COLUMN_KERNEL) == -1 and e.info(INFO_VERTICAL_KERNELS) == -1      # nothing was launched
        for ix in (0, 1, 2):
            st, t = e.download_state(ix), e.download_tracers(ix)
            assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(st, before[ix][0])), (mode, ix)
            assert all(np.array_equal(a, b) for a, b in zip(t, before[ix][1])), (mode, ix)
    finally:
        e.close()


def test_whole_steps_at_157_levels_vs_oracle():
    """STEPS_SHAPE = (157 levels, no tracers), above every walk threshold of the vertical kernels: two ARS343 steps and one Strang step, and two ARK232
    steps (StepImplicitTermsExplicitly: the level-parallel terms kernel, 416 L + 4 504 > 64 KB), on the node-unique and on the element-major layout
    against the oracle, bit for bit.  The explicit-stage walk, the hyperviscosity walk and the DSS ride along at this level count; the column
    solve is the lane-group kernel's (3 x 158 = 474 of its ring's 480 doubles)."""
    from oracle_lib import Oracle
    from tempestmodel_amd.engine import Engine
    L, _ = STEPS_SHAPE
    g, states = gu.make_grid(3, L, 6)
    assert max(Engine.scheme_instances(s_) for s_ in ("ars343", "strang", "ark232")) <= STEPS_NINST
    o = Oracle(g, ninst=STEPS_NINST); o.set_state(0, states)
    assert o.step_ars343(100.0) == 0
    smooth = o.get_state(0)
    programs = {"ars343+strang": [("ars343", False), ("ars343", False), ("strang", True)], "ark232": [("ark232", False), ("ark232", False)]}
    want = {}
    for key, prog in programs.items():
        o.set_state(0, smooth)
        for scheme, first in prog:
            assert o.step(scheme, 100.0, first=first) == 0, (key, scheme)
        want[key] = o.get_state(0)
        assert _finite(want[key]) and max(_errs(want[key], smooth)) > 0.0, key
    bad = []
    for unique in (True, False):
        e = Engine(g, n_instances=STEPS_NINST, options={} if unique else {"unique_layout": 0})
        try:
            for key, prog in programs.items():
                _scrub(e, states, 37.0)
                e.upload_state(0, smooth)
                for scheme, first in prog:
                    e.step(scheme, 100.0, first=first)
                e.sync()
                assert e.info(12) == (1 if unique else 0) and (unique or e.info(13) == 0), (key, unique)      # TMX_INFO_UNIQUE_LAYOUT, _UNIQUE_INSTANCES
                assert (e.info(INFO_COLUMN_KERNEL), e.info(INFO_COLUMN_VARIANT)) == (2, 0), (key, unique)
                if key == "ark232":
                    assert (e.info(INFO_VERTICAL_KERNELS) >> 24) & 0xfff == 0, (key, unique)      # the terms kernel: level-parallel at 157 levels
                errs = _errs(e.download_state(0), want[key])
                print("L %d %s %s: stage kernel %#x hyperviscosity kernel %d" % (L, key, "node-unique" if unique else "element-major", e.info(22), e.info(23)), errs)
                if not max(errs) == 0.0:
                    bad.append((key, unique, errs))
        finally:
            e.close()
    assert not bad, bad


# (L, tracers) of the multiply + subtract case below.  At (7, 4) the oracle's two modes of the band LU leave different tracers behind
# V.StepImplicit (checked on the CPU, where the oracle runs: 2.1e-17 of the tracers' maximum, state 3.4e-16; at (30, 4) 1.5e-16 and 8.3e-15),
# so the smallest L of {7, 30} is taken.  Behind StepImplicitTermsExplicitly the two modes leave the SAME tracers and state at both level
# counts (0.0): there W is not the column solve's, and with dt = 0.7 the tridiagonal matrix is so dominated by 1/dt that a - l u rounds
# alike either way.  So what separates the modes in this case reaches the tracers through the W of the column solve as well.
SHAPE_NOFMA = (7, 4)


def test_implicit_tracer_column_update_with_the_multiply_subtract_band_lu():
    """Option "lu_fma" = 0 (band-LU updates as multiply and subtract, rounded separately) in the tracers' column solve, by the row-lane
    kernel and by its one-row-lane form: state and tracers equal the oracle's under orc_set_lu_fma(0), and behind V.StepImplicit the
    oracle's two modes differ at this shape (SHAPE_NOFMA: what does and what does not separate them here)."""
    from oracle_lib import lib
    from tempestmodel_amd.engine import Engine
    L, nt = SHAPE_NOFMA
    g, _, tr = _case(L, nt)
    calls = ("v_step_implicit", "v_step_implicit_terms_explicitly")
    fused = _oracle_calls(L, nt, calls)
    bad = []
    try:
        lib().orc_set_lu_fma(0)
        want = _oracle_calls(L, nt, calls)
        for name, (_, ft), (_, wt) in zip(calls, fused, want):
            diff = max(_terrs(ft, wt))
            print("oracle, fused against multiply + subtract:", name, diff)
            assert diff < float("inf"), name
            if name == "v_step_implicit":
                assert EXACT < diff, name
        for rows in (1, 0):
            e = Engine(g, options={"vt_rows": rows, "lu_fma": 0})
            try:
                got = _device_calls(e, L, nt, calls)
            finally:
                e.close()
            assert max(_terrs(got[0][1], tr)) > 0.0 and max(_terrs(got[1][1], tr)) > 0.0, rows
            _compare(bad, (L, nt, "lu_fma", 0, "vt_rows", rows), calls, got, want)
    finally:
        lib().orc_set_lu_fma(1)
    assert not bad, bad
