"""The output kernels (restart image, output interpolation) across level counts, point counts and ranks.

k_active_state_image strides 64 lanes over the L and L + 1 entries of a column and stages one variable of 64 columns in (L + 1) x 65
doubles of LDS; k_interp_state / k_interp_tracers run one thread per (point, output level) in blocks of 256 points.  Their fixtures fix
one shape each (ne3 L6 with two tracers; ne4 L6 with 74 points, no topography), so the shapes at which something changes are run here.
The image is DEFINED by the uploaded arrays plus two operator applications, the interpolation has the C oracle and a long-double
restatement of the reference's statements: no new fixture.  Inputs: tests/levels_common.py (qualified on the CPU by
tests/test_levels_inputs_host.py)."""
import numpy as np
import pytest
import golden_util as gu
import levels_common as lc

pytestmark = pytest.mark.gpu

INFO_UNIQUE_INSTANCES = 13      # tmx_info (include/tempest_mi355x.h)
EPS = float(np.finfo(np.float64).eps)

SENTINEL = 12345.678            # what an instance holds where no image may be unpacked

IMAGE_CASES = [(3, 3, 0), (2, 6, 1), (3, 63, 0), (3, 64, 3), (3, 65, 1), (3, 93, 0), (3, 94, 2)]


def _split(img, P, L, nt):
    """header word, padding, node [5][na][nb][L], redge [5][na][nb][L+1], tracers [nt][na][nb][L] of one image"""
    nn = P.na * P.nb
    assert img.size == 8 * (1 + 5 * nn * L + 5 * nn * (L + 1) + nt * nn * L)
    body = img[8:].view(np.float64)
    node = body[:5 * nn * L].reshape(5, P.na, P.nb, L)
    redge = body[5 * nn * L:5 * nn * (2 * L + 1)].reshape(5, P.na, P.nb, L + 1)
    trc = body[5 * nn * (2 * L + 1):].reshape(nt, P.na, P.nb, L)
    return int(img[:4].view(np.int32)[0]), img[4:8], node, redge, trc


def _halo_is_zero(a):
    return not a[:, 0].any() and not a[:, -1].any() and not a[:, :, 0].any() and not a[:, :, -1].any()


def _interior_equal(a, b):
    return np.array_equal(a[..., 1:-1, 1:-1, :], b[..., 1:-1, 1:-1, :])


def _dot_bound(op, x, got):
    """max over the entries of |got - op x| / (gamma_4 sum |c_i x_i|), op applied along the last axis in np.longdouble: the forward
    bound of a dot product of at most four terms in any order of summation.  <= 1 passes; rows of the operator have <= 4 non-zeros."""
    assert int(np.count_nonzero(op, axis=1).max()) <= 4
    ld = np.longdouble
    want = np.einsum("kl,...l->...k", op.astype(ld), x.astype(ld))
    mag = np.einsum("kl,...l->...k", np.abs(op).astype(ld), np.abs(x).astype(ld))
    gamma4 = ld(4 * EPS / 2) / (1 - ld(4 * EPS / 2))      # 4 u / (1 - 4 u) with the unit roundoff u = eps / 2
    err = np.abs(got.astype(ld) - want)
    assert not (err[mag == 0] != 0).any()
    return float(np.max(err[mag > 0] / (gamma4 * mag[mag > 0]))) if (mag > 0).any() else 0.0      # (V is identically zero on some patches)


@pytest.mark.parametrize("ne,L,nt", IMAGE_CASES, ids=["ne%d_L%d_nt%d" % c for c in IMAGE_CASES])
def test_restart_image_is_the_uploaded_arrays(ne, L, nt):
    """tmx_pack_active_state right after the upload (no step), 6 patches; ne2 = 64 columns per patch, one exactly full tile, ne3 = 144,
    the last tile holding one element:

        (3, 3, 0)                             no tracers, the engine's minimum of levels
        (2, 6, 1)                             one exactly full tile per patch
        (3, 63, 0), (3, 64, 3), (3, 65, 1)    one trip of the 64-lane stride over both L and L + 1 / one and two / two and two
        (3, 93, 0), (3, 94, 2)                the two sides of the opt-in to more than 48 KB of dynamic LDS: (L + 1) x 65 x 8 =
                                              48 880 and 49 400 bytes

    Expected, from the UPLOADED arrays: header word = patch index, four zero bytes; the four prognostic node arrays, W on interfaces
    and the tracers bit-equal to the upload on the interior; halo ring zero; rho*theta and rho on interfaces zero (no tracked surface
    slots).  The derived arrays (W on levels, U and V on interfaces) are bit-equal to tmx_download_state's and within the forward
    bound of a four-term dot product, gamma_4 sum |c_i x_i|, of the long-double application of the grid's own InterpREdgeToNode /
    InterpNodeToREdge rows to the upload (printed: the largest error in units of that bound).  Unpacking into another instance and
    into a second engine reproduces the interior bits of the upload, and writes no column of another patch: the first goes through
    the patches in descending order, the second unpacks patches 0, 2, 4 into a sentinel-filled instance and finds 1, 3, 5 untouched
    (a lane one past the ragged last tile of ne3 would write the first column of the next patch; going up the patches on one stream,
    the next unpack would cover that up).

    Shown to bite in a scratch build: `cl < a.ncp` -> `cl <= a.ncp` in k_active_state_image fails both unpack checks at every ne3
    case (patch 1 at its first column) and passes ne2, whose last tile is full."""
    from tempestmodel_amd.engine import Engine
    g, states = gu.make_grid(ne, L, 6, ntracers=nt)
    st, tr = lc.image_state(g, states, seed=L)
    n2e, e2n = g.ops["interp_node_to_redge"][0], g.ops["interp_redge_to_node"][0]
    e = Engine(g)
    e2 = None
    try:
        e.upload_state(0, st)
        if nt:
            e.upload_tracers(0, tr)
        down = e.download_state(0)
        images, worst = [], 0.0
        for P, (un, ue), (dn, de) in zip(g.patches, st, down):
            img = e.pack_active_state(P.index, 0)
            images.append(img)
            ix, pad, node, redge, trc = _split(img, P, L, nt)
            assert ix == P.index and not pad.any()
            assert _interior_equal(node[[0, 1, 2, 4]], un[[0, 1, 2, 4]]) and _interior_equal(redge[3], ue[3]), P.index
            if nt:
                assert _interior_equal(trc, tr[P.index]), P.index
            assert _halo_is_zero(node) and _halo_is_zero(redge) and (nt == 0 or _halo_is_zero(trc)), P.index
            assert not redge[[2, 4]].any(), P.index
            assert _interior_equal(node[3], dn[3]) and _interior_equal(redge[[0, 1]], de[[0, 1]]), P.index
            for bound in (_dot_bound(e2n, ue[3][1:-1, 1:-1], node[3][1:-1, 1:-1]), _dot_bound(n2e, un[0][1:-1, 1:-1], redge[0][1:-1, 1:-1]),
                          _dot_bound(n2e, un[1][1:-1, 1:-1], redge[1][1:-1, 1:-1])):
                worst = gu.worse(worst, bound)      # (a NaN bound becomes inf: max(worst, nan) would drop it)
        print("image ne%d L%d nt%d: derived arrays within %.3f of the gamma_4 bound" % (ne, L, nt, worst))
        assert worst <= 1.0
        # unpack, another instance: the patches in DESCENDING order, so that a lane that runs past its patch's last column damages a
        # patch already unpacked and nothing repairs it before the download
        for P, img in reversed(list(zip(g.patches, images))):
            e.unpack_active_state(P.index, 3, img)
        e.sync()
        for (gn, ge), (un, ue) in zip(e.download_state(3), st):
            assert _interior_equal(gn[[0, 1, 2, 4]], un[[0, 1, 2, 4]]) and _interior_equal(ge[3], ue[3])
        if nt:
            assert all(_interior_equal(a, b) for a, b in zip(e.download_tracers(3), tr))
        # unpack, a second engine whose instance holds a sentinel: only patches 0, 2, 4 are unpacked, these carry the upload and
        # their neighbours in the column order, 1, 3, 5, still hold the sentinel in every stored column, the first and last included
        e2 = Engine(g)
        e2.upload_state(0, [(np.full_like(un, SENTINEL), np.full_like(ue, SENTINEL)) for un, ue in st])
        if nt:
            e2.upload_tracers(0, [np.full_like(t, SENTINEL) for t in tr])
        for P, img in zip(g.patches, images):
            if P.index % 2 == 0:
                e2.unpack_active_state(P.index, 0, img)
        e2.sync()
        got, got_tr = e2.download_state(0), (e2.download_tracers(0) if nt else None)
        for P, (gn, ge), (un, ue) in zip(g.patches, got, st):
            if P.index % 2 == 0:
                assert _interior_equal(gn[[0, 1, 2, 4]], un[[0, 1, 2, 4]]) and _interior_equal(ge[3], ue[3]), P.index
                assert nt == 0 or _interior_equal(got_tr[P.index], tr[P.index]), P.index
            else:
                assert (gn[[0, 1, 2, 4], 1:-1, 1:-1] == SENTINEL).all() and (ge[3, 1:-1, 1:-1] == SENTINEL).all(), P.index
                assert nt == 0 or (got_tr[P.index][:, 1:-1, 1:-1] == SENTINEL).all(), P.index
    finally:
        e.close()
        if e2 is not None:
            e2.close()


def test_restart_image_carries_the_tracked_surface_slots():
    """(ne3, L = 5, no tracers) with the tracked surface slots (set_physics_inputs(None)): after three steps with the Held-Suarez
    forcing the image carries the two interface-level-0 entries (rho*theta and rho) tmx_download_state returns, and a second engine
    that only ever saw the images continues for two more forced steps bit-identically, the slots included."""
    from tempestmodel_amd.engine import Engine
    L = 5
    g, states = gu.make_grid(3, L, 6)
    e, e2 = Engine(g), None
    try:
        e.set_physics_inputs(None)
        e.upload_state(0, states)
        for _ in range(3):
            e.step_ars343(100.0); e.held_suarez(0, 100.0)
        e.sync()
        down = e.download_state(0)
        images = [e.pack_active_state(P.index, 0) for P in g.patches]
        for P, img, (dn, de) in zip(g.patches, images, down):
            _, _, node, redge, _ = _split(img, P, L, 0)
            assert _interior_equal(node, dn) and _interior_equal(redge[[0, 1, 3]], de[[0, 1, 3]])
            assert np.array_equal(redge[[2, 4], 1:-1, 1:-1, 0], de[[2, 4], 1:-1, 1:-1, 0]) and (redge[[2, 4], 1:-1, 1:-1, 0] > 0.0).all()
            assert not redge[[2, 4], :, :, 1:].any()
        e2 = Engine(g)
        e2.set_physics_inputs(None)
        for P, img in zip(g.patches, images):
            e2.unpack_active_state(P.index, 0, img)
        for eng in (e, e2):
            for _ in range(2):
                eng.step_ars343(100.0); eng.held_suarez(0, 100.0)
            eng.sync()
        a, b = e.download_state(0), e2.download_state(0)
        assert max(gu.prognostic_errors(b, a)) == 0.0
        for (an, ae), (bn, be) in zip(a, b):
            assert np.array_equal(ae[[2, 4], 1:-1, 1:-1, 0], be[[2, 4], 1:-1, 1:-1, 0])
        assert 1e-6 < max(gu.prognostic_errors(a, down)) < float("inf")      # the two steps moved the state
    finally:
        e.close()
        if e2 is not None:
            e2.close()


def test_restart_image_of_a_node_unique_instance():
    """After two steps on an engine eligible for the node-unique layout the instance is held in that form (info(UNIQUE_INSTANCES) > 0
    before packing): its image is the one of a unique_layout = 0 engine, byte for byte."""
    from tempestmodel_amd.engine import Engine
    g, states = gu.make_grid(3, 7, 6)
    u, d = Engine(g, options={"unique_layout": 1}), Engine(g, options={"unique_layout": 0})
    try:
        for e in (u, d):
            e.upload_state(0, states)
            e.step_ars343(100.0); e.step_ars343(100.0)
        assert u.info(INFO_UNIQUE_INSTANCES) > 0 and d.info(INFO_UNIQUE_INSTANCES) == 0
        for P in g.patches:
            a, b = u.pack_active_state(P.index, 0), d.pack_active_state(P.index, 0)
            assert np.array_equal(a, b), P.index
            assert _split(a, P, 7, 0)[2][:, 1:-1, 1:-1].any()
    finally:
        u.close(); d.close()


# ---- output interpolation ----

NPTS = [1, 255, 256, 257, 600]      # one thread; one block less one lane, full, plus one lane; three blocks, the last ragged


def _ulps(got, want):
    """largest |got - want| per field in units of the spacing of the doubles at |want|"""
    return [float(np.max(np.abs(got[c] - want[c]) / np.spacing(np.maximum(np.abs(want[c]), np.finfo(np.float64).tiny)))) for c in range(len(want))]


@pytest.mark.parametrize("ne,L,npatch,case,ntr,dt", lc.INTERP_GRIDS, ids=lc.INTERP_IDS)
def test_output_interpolation_vs_oracle_and_long_double(ne, L, npatch, case, ntr, dt):
    """tmx_interp_state / tmx_interp_tracers on levels_common.interp_state with levels_common.interp_points, npts in {1, 255, 256, 257,
    600} x nreta in {1, 4}, all four (include_reference_state, convert_to_primitive) combinations, only_variables_at 1 and 2 once each,
    the tracers where the grid has some; grids (ne3, L5, 6 patches), (ne4, L70, 24 patches) and the Schar mountain at ne3 with the
    smallest level count the engine accepts (3).  d_xi R differs between the nodes of an element by 1.0e-2, 7.8e-3 and 4.5e-3 relative
    on the three grids (asserted on the CPU), so that dividing W by the FIRST node's value (GridPatchCSGLL.cpp:1665) shows on each.

      (i)  the C oracle on identical inputs: the first run on an MI355X gave 0 ulps in every field of every case, so this asserts
           np.array_equal;
      (ii) the np.longdouble restatement of GridPatchCSGLL.cpp:1644-1760 (levels_common.interp_longdouble): per field and case the
           device is at most twice as far from it as the oracle is in the same test, with a floor of 8 eps; distances are relative to
           max |field| BEFORE the reference state is subtracted.  Measured on an MI355X, largest over fields and cases per grid:
           oracle 6.7e-16 (ne3 L5), 9.3e-16 (ne4 L70), 7.4e-16 (Schar), tracers up to 9.6e-16; with (i)
           exact the device's are the same numbers.  Both are printed.  The all-zero operator row gives exactly 0.0.

    Shown to bite in a scratch build: `p.g2d[G2_DRX * NS + col0]` -> `... + col0 + 5]` in k_interp_state (d_xi R of another node of
    the element; in bounds) fails (i) in W on all three grids at the first case with a non-trivial operator row (1 point, 4 rows)."""
    from tempestmodel_amd.engine import Engine
    from oracle_lib import Oracle
    g, states = gu.make_grid(ne, L, npatch, case=case, ntracers=ntr)
    st, tr = lc.interp_state(g, states, dt=dt)
    a = float(g.phys.earth_radius)
    o = Oracle(g); o.set_state(0, st)
    if ntr:
        o.set_tracers(0, tr)
    e = Engine(g)
    try:
        e.upload_state(0, st)
        if ntr:
            e.upload_tracers(0, tr)
        e.set_reference_state()
        worst_ulps, worst_dev, worst_orc = 0.0, 0.0, 0.0
        for npts in NPTS:
            for nreta in (1, 4):
                pts = lc.interp_points(g, npts, nreta, seed=npts + nreta)
                plan = e.interp_create(pts)
                try:
                    cases = [(0, inc, prim) for inc in (True, False) for prim in (True, False)]
                    if (npts, nreta) == (257, 4):
                        cases += [(1, True, False), (2, False, True)]
                    for only, inc, prim in cases:
                        got = e.interp_state(plan, 0, only, inc, prim, a)
                        orc = o.interpolate_state(0, pts, only, inc, prim, a)
                        want, _ = lc.interp_longdouble(g, st, None, pts, only, inc, prim, a)
                        full, _ = lc.interp_longdouble(g, st, None, pts, only, True, prim, a)
                        ulps = _ulps(got, orc)
                        d_dev, d_orc = lc.field_distance(got, want, full), lc.field_distance(orc, want, full)
                        print("interp %s npts %d nreta %d only %d ref %d prim %d: ulps vs oracle %s; vs long double: device %s oracle %s" % (
                            case, npts, nreta, only, inc, prim, ulps, ["%.1e" % v for v in d_dev], ["%.1e" % v for v in d_orc]))
                        for v in ulps:
                            worst_ulps = gu.worse(worst_ulps, v)
                        for v, w in zip(d_dev, d_orc):
                            worst_dev, worst_orc = gu.worse(worst_dev, v), gu.worse(worst_orc, w)
                        assert np.array_equal(got, orc), (npts, nreta, only, inc, prim, ulps)
                        for c in range(5):
                            assert np.isfinite(d_orc[c]) and d_dev[c] <= max(2.0 * d_orc[c], 8.0 * EPS), (npts, nreta, only, inc, prim, c, d_dev[c], d_orc[c])
                        if nreta == 4:
                            assert not got[:, 2].any() and np.isfinite(got).all()
                        if only == 1:
                            assert not got[3].any() and got[0].any()
                        if only == 2:
                            assert not got[[0, 1, 2, 4]].any() and got[3].any()
                    if ntr:
                        got, orc = e.interp_tracers(plan, 0), o.interpolate_tracers(0, pts)
                        _, want = lc.interp_longdouble(g, st, tr, pts)
                        d_dev, d_orc = lc.field_distance(got, want, want), lc.field_distance(orc, want, want)
                        print("interp %s npts %d nreta %d tracers: ulps vs oracle %s; vs long double: device %s oracle %s" % (
                            case, npts, nreta, _ulps(got, orc), ["%.1e" % v for v in d_dev], ["%.1e" % v for v in d_orc]))
                        assert np.array_equal(got, orc), (npts, nreta)
                        assert all(np.isfinite(d_orc[c]) and d_dev[c] <= max(2.0 * d_orc[c], 8.0 * EPS) for c in range(ntr)), (npts, nreta, d_dev, d_orc)
                        assert got[:, 0].any() and (nreta == 1 or not got[:, 2].any())
                finally:
                    e.interp_destroy(plan)
        print("interp %s: worst ulps vs oracle %g; worst distance to long double: device %.2e, oracle %.2e" % (case, worst_ulps, worst_dev, worst_orc))
    finally:
        e.close()


@pytest.mark.parametrize("ne,L,npatch,case,ntr,dt", lc.INTERP_GRIDS[:2], ids=lc.INTERP_IDS[:2])
def test_output_interpolation_on_two_rank_engines(ne, L, npatch, case, ntr, dt):
    """Two loopback rank engines share one plan description (600 points, 4 output levels): a point on a patch of the other rank has
    no column there (col0 = -1) and comes back as 0.0 in every field, so every point is zero on exactly one rank, and the rank
    that owns it returns the single engine's bits -- state (reference state removed, primitive) and tracers."""
    from tempestmodel_amd.engine import Engine, default_owner
    g, states = gu.make_grid(ne, L, npatch, case=case, ntracers=ntr)
    st, tr = lc.interp_state(g, states, dt=dt)
    a = float(g.phys.earth_radius)
    pts = lc.interp_points(g, 600, 4, seed=7)
    owner = default_owner(npatch, 2)
    engines = []
    try:
        for r in (None, 0, 1):
            e = Engine(g) if r is None else Engine(g, rank=r, n_ranks=2, owner=owner)
            engines.append(e)
            e.upload_state(0, st); e.upload_tracers(0, tr)
            e.set_reference_state()
        out = []
        for e in engines:
            plan = e.interp_create(pts)
            try:
                out.append((e.interp_state(plan, 0, 0, False, True, a), e.interp_tracers(plan, 0)))
            finally:
                e.interp_destroy(plan)
        rank_of = np.asarray(owner)[pts["patch"]]
        assert 100 < int(np.count_nonzero(rank_of == 0)) < 500
        rows = [0, 1, 3]                                  # (row 2 of the operators is all zero on every rank)
        for which in (0, 1):
            single = out[0][which]
            assert single[:, rows].any(axis=(0, 1)).all()      # no point is zero by itself
            for r in (0, 1):
                got = out[1 + r][which]
                mine = rank_of == r
                assert np.array_equal(got[..., mine], single[..., mine]), (which, r)
                assert not got[..., ~mine].any(), (which, r)
    finally:
        for e in engines:
            e.close()
