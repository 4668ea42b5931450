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
which the implicit branch has a reference; the explicit branch's matrix is the diagonal, which the three rows hold."""
import functools
import numpy as np
import pytest
import golden_util as gu
from parity_common import EXACT, UDIFF
from test_gpu_stage_walk_segments import _errs, _terrs, _finite

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4), (7, 4), (7, 1)]
# (see above); 35 and 36 levels: the two sides of the one-row-lane kernel's switch from 64 to 32 columns per workgroup in the all-columns
# form -- its working set, (9L + 3) doubles per column, fits the 160 KB of a CU 64 times up to L = 35
SHAPES_IMPLICIT = [(4, 4), (7, 4), (7, 1), (35, 1), (36, 1)]
DT = 0.7


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


def _device_calls(e, L, nt, calls):
    _, rough, tr = _case(L, nt)
    e.upload_state(0, rough); e.upload_tracers(0, tr)
    got = []
    for ix, name in ((1, calls[0]), (2, calls[1])):
        e.copy_data(0, ix)
        getattr(e, name)(0, ix, DT)
        e.sync()
        got.append((e.download_state(ix), e.download_tracers(ix)))
    return got


def _compare(bad, tag, calls, got, want):
    for name, (gs, gt), (ws, wt) in zip(calls, got, want):
        errs, terrs = _errs(gs, ws), _terrs(gt, wt)
        print(tag, name, errs, terrs)
        if not (max(errs) <= EXACT and max(terrs) <= EXACT):
            bad.append((tag, name, errs, terrs))


@pytest.mark.parametrize("ud", [True, False], ids=["udiff", "plain"])
@pytest.mark.parametrize("L,nt", SHAPES, ids=["L%d_nt%d" % s for s in SHAPES])
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
            got = _device_calls(e, L, nt, calls)
        finally:
            e.close()
        assert max(_terrs(got[0][1], tr)) > 0.0, opts      # the update changed the tracers
        _compare(bad, (L, nt, ud, opts), calls, got, want)
    assert not bad, bad


@pytest.mark.parametrize("L,nt", SHAPES_IMPLICIT, ids=["L%d_nt%d" % s for s in SHAPES_IMPLICIT])
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
            got = _device_calls(e, L, nt, calls)
        finally:
            e.close()
        assert max(_terrs(got[0][1], tr)) > 0.0 and max(_terrs(got[1][1], tr)) > 0.0, rows      # both updates changed the tracers
        _compare(bad, (L, nt, "vt_rows", rows), calls, got, want)
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
