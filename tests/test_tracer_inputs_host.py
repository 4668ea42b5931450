"""The inputs of tests/tracer_inputs_common.py make both FilterNegativeTracers variants act in every one of their cases: asserted here on
the C oracle and in numpy alone, no device.  Three things per shape of tests/test_gpu_tracer_transport_shapes.py: every oracle result
that file compares with is finite in the interior; the cases of both filters (tracer_inputs_common's header) occur in every patch,
counted; and the numpy restatement of both filters is bit-equal to the oracle's export -- the plain reference the GPU file also uses.

The counts are conditions.  (3, 1) has one tracer, of kind 0 (signs flipped node by node), which cannot hold an all-zero element or
column and in practice no element of 16 non-positive nodes (0.3^16): those cases are asserted ABSENT there and present at every other
shape, the remaining cases at every shape."""
import numpy as np
import pytest
import golden_util as gu
import tracer_inputs_common as tc

IDS = ["L%d_nt%d" % s for s in tc.SHAPES]


@pytest.mark.parametrize("L,nt", tc.SHAPES, ids=IDS)
@pytest.mark.parametrize("vertical", [False, True], ids=["horizontal", "vertical"])
def test_filter_cases_occur_in_every_patch_and_restatement_equals_export(L, nt, vertical):
    """The exported filter applied to the input itself: the numpy restatement gives the same doubles (signs of zero included: every zero
    is +0.0), and per patch, over the tracers of kinds 0 and 1 (horizontal) or 0 and 2 (vertical), every case occurs at least once."""
    g, _, _, _, _ = tc.case(L, nt)
    tin, tout, _ = tc.want_filters(L, nt, vertical)
    again = (tc.filter_v_numpy if vertical else tc.filter_h_numpy)(g, tin)
    keep = (0, 2) if vertical else (0, 1)
    counts = []
    for P, a, b, c in zip(g.patches, tin, tout, again):
        assert np.isfinite(b).all(), P.index
        assert np.array_equal(b, c), P.index
        assert not np.signbit(b[b == 0.0]).any() and not np.signbit(c[c == 0.0]).any(), P.index
        assert np.array_equal(a[:, [0, -1]], b[:, [0, -1]]) and np.array_equal(a[:, :, [0, -1]], b[:, :, [0, -1]]), P.index      # the halo ring is not touched
        cin, cout = tc.cells_of_tracers(a, vertical, keep), tc.cells_of_tracers(b, vertical, keep)
        m = tc.class_masks(cin)
        assert (cout[m["all <= 0"] | m["all zero"]] == 0.0).all(), P.index      # r = -inf and r = NaN never reach a product
        counts.append(tc.class_counts(cin, cout))
    table = {k: [c[k] for c in counts] for k in tc.CLASSES}
    print("L %d, %d tracers, %s filter, units per patch:" % (L, nt, "vertical" if vertical else "horizontal"), table)
    absent = []
    if nt == 1:      # kind 0 alone (see the module's docstring)
        absent = ["all zero"] if vertical else ["all <= 0", "all zero"]
    for k in tc.CLASSES:
        if k in absent:
            assert max(table[k]) == 0, (k, table[k])
        else:
            assert min(table[k]) >= 1, (k, table[k])


@pytest.mark.parametrize("L,nt", tc.SHAPES, ids=IDS)
def test_percall_results_are_finite_clip_and_leave_negatives(L, nt):
    """(a), (b): every instance the GPU file compares is finite in the interior, differs from the input and holds exact zeros and
    negative values; with dt = 0 H.StepExplicit IS the horizontal filter of the input (base - 0 * (...) with finite fluxes), bit for bit
    the export."""
    for which in ("rough", "smooth"):
        w = tc.want_percall(L, nt, which)
        for ix in (1, 2, 3, 4, 5):
            assert tc.interior_finite(w[ix]), (which, ix)
        for ix in (1, 3, 5) + ((2,) if L >= 4 else ()):
            assert min(gu.tracer_errors(w[ix][1], w[0][1])) > 0.0, (which, ix)      # every tracer changed
            z, n = tc.fractions(w[ix][1])
            print("L %d nt %d %s instance %d: %.0f %% zeros, %.0f %% negative" % (L, nt, which, ix, 100 * z, 100 * n))
            assert (z > 0.0 or ix == 5) and n > 0.0, (which, ix, z, n)      # (the combination is no filter's output: it need not hold a zero)
    w0 = tc.want_percall(L, nt, "smooth", 0.0)
    _, tout, _ = tc.want_filters(L, nt, False)
    for a, b in zip(w0[1][1], tout):
        assert np.array_equal(a[:, 1:-1, 1:-1], b[:, 1:-1, 1:-1])
    assert tc.interior_finite(w0[3]) and tc.interior_finite(w0[4])
    z, n = tc.fractions(w0[3][1])
    assert z > 0.0 and n > 0.0


def test_planted_negative_zeros_come_back_positive():
    """(c): the -0.0 entries planted for the direct vertical-filter test leave the oracle's filter as +0.0 (the reference stores = 0.0),
    and the restatement agrees."""
    for L, nt in tc.SHAPES:
        g = tc.case(L, nt)[0]
        tin, tout, where = tc.want_filters(L, nt, True, plant=True)
        for a, b, c, ix in zip(tin, tout, tc.filter_v_numpy(g, tin), where):
            assert np.signbit(a[tuple(ix)]).all() and (a[tuple(ix)] == 0.0).all()
            assert not np.signbit(b[tuple(ix)]).any() and (b[tuple(ix)] == 0.0).all()
            assert np.array_equal(b, c) and not np.signbit(c[c == 0.0]).any()


@pytest.mark.parametrize("key", tc.VISC_KEYS)
def test_viscosity_cases_are_finite_and_do_what_they_say(key):
    """(d): finite results; orders 2 and 4 (also unscaled) change and clip the tracers, order 0 and nu = 0 copy them (the Schar
    mountain's Rayleigh layer then still relaxes the state)."""
    (g, _, st, tr, _), kw, dt = tc.visc_case(key)      # (st: the rough state the call runs on)
    upd, work, steps = tc.want_visc(key)
    assert tc.interior_finite(upd) and all(tc.interior_finite(s) for s in steps), key
    copy = key.endswith("order0") or key == "nu0"
    errs = gu.tracer_errors(upd[1], tr)
    if copy:
        assert max(errs) == 0.0, (key, errs)
    else:
        assert min(errs) > 0.0, (key, errs)
        z, n = tc.fractions(upd[1])
        assert z > 0.0 and n > 0.0, (key, z, n)
    if key.startswith("schar_"):
        assert getattr(g, "has_rayleigh_friction", False)
        assert max(gu.prognostic_errors(upd[0], st)) > 0.0, key      # the relaxation follows the copy
    if key == "reflen0":
        other = tc.want_visc("order2")      # (any other configuration of the same shape: the grids differ in reference_length alone)
        assert g.reference_length == 0.0 and tc.case(*tc.SHAPE_VISC)[0].reference_length != 0.0
        assert max(gu.tracer_errors(upd[1], other[0][1])) > 0.0


@pytest.mark.parametrize("L,nt", tc.SHAPES_UDIFF, ids=["L%d_nt%d" % s for s in tc.SHAPES_UDIFF])
def test_uniform_diffusion_results_are_finite(L, nt):
    """(e): every call changes the tracers; everything finite."""
    g, st, rough, tr, _ = tc.case(L, nt, name="smallplanet")
    calls, steps = tc.want_udiff(L, nt)
    for name, snap in calls:
        assert tc.interior_finite(snap), name
        assert min(gu.tracer_errors(snap[1], tr)) > 0.0, name
    for scheme, first, snap in steps:
        assert tc.interior_finite(snap), (scheme, first)
    z, n = tc.fractions(calls[0][1][1])
    assert z > 0.0 and n > 0.0


def test_whole_steps_are_finite():
    """(f), (g): finite after every step, zeros and negatives in the tracers."""
    runs = [(L, nt, prog, 3, 6) for L, nt in tc.SHAPES_STEPS for prog in ("ars343", "strang")] + [(7, 4, "ark232", 3, 6)]
    runs.append(tc.SHAPE_RANKS + ("ars343", 12, 24))
    for L, nt, prog, ne, npatch in runs:
        for snap in tc.want_steps(L, nt, prog, ne=ne, npatch=npatch):
            assert tc.interior_finite(snap), (L, nt, prog, ne)
            z, n = tc.fractions(snap[1])
            assert z > 0.0 and n > 0.0, (L, nt, prog, ne, z, n)
