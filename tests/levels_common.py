"""Input builders of the tests that run the kernels outside the stepper across level counts (tests/test_gpu_physics_levels.py,
tests/test_gpu_output_levels.py): column physics, restart image, output interpolation.  Every grid is golden_util.make_grid's, every
input is seeded; what makes an input worth running (rain sub-cycles that differ inside a wavefront, both sides of the sigma = 0.7 and
of the 200 K branch, W != 0, state away from the reference state) is asserted on the C oracle and in numpy alone by
tests/test_levels_inputs_host.py, without a device."""
import math
import numpy as np
import golden_util as gu

KESSLER_LEVELS = [3, 5, 6, 31, 32, 37, 40, 41, 60]
HELD_SUAREZ_LEVELS = [3, 4, 5, 30, 61]
# output interpolation: (ne, L, patches, case, tracers, dt of the oracle step behind interp_state).  The Schar mountain lives on the
# reduced-radius sphere (a = 12.7 km, so ne3 elements are about 3 km wide): one ARS343 step of 100 s does not stay finite there (the
# oracle returns NaN; at 10 s and below it is finite), so that grid steps 0.5 s.  L = 3 is the smallest count the engine accepts.
INTERP_GRIDS = [(3, 5, 6, "jw", 2, 100.0), (4, 70, 24, "jw", 2, 100.0), (3, 3, 6, "schar", 0, 0.5)]
INTERP_IDS = ["ne3_L5", "ne4_L70_p24", "schar_ne3_L3"]
KESSLER_DT_L3 = 800.0      # at L = 3 the rain loop splits only from here on ({1, 2}; one pass at 400 s): run there in addition
GLL4 = (-1.0, -1.0 / math.sqrt(5.0), 1.0 / math.sqrt(5.0), 1.0)      # np = 4 GLL nodes on [-1, 1]


def stored_columns(grid):
    """(patch, i, j) of every stored column in the device's order: patch by patch, element by element (alpha-major), 4 x 4 nodes of
    an element (alpha-major) -- 64 consecutive ones are what one wavefront of a column kernel holds."""
    out = []
    for P in grid.patches:
        nea, neb = (P.na - 2) // 4, (P.nb - 2) // 4
        ea, eb, i, j = np.meshgrid(np.arange(nea), np.arange(neb), np.arange(4), np.arange(4), indexing="ij")
        out.append(np.stack([np.full(ea.size, P.index), (1 + 4 * ea + i).ravel(), (1 + 4 * eb + j).ravel()], 1))
    return np.concatenate(out, 0)


def moist_supercell(ne, L, npatch=6, seed=0):
    """Grid, state and tracers (RhoQv, RhoQc, RhoQr) for the Kessler kernels: the supercell configuration's resting column with seeded
    moisture -- vapour decaying with height, cloud everywhere, rain of a very different amount from one column to the next (a^4 with
    one a ~ U(0,1) per column), so that the CFL limit of the rain loop splits neighbouring columns differently."""
    g, states = gu.make_grid(ne, L, npatch, ztop=20000.0, case="supercell")
    rng = np.random.default_rng(seed)
    decay = np.exp(-np.arange(L) / (L / 3.0))
    tracers = []
    for P, (node, _) in zip(g.patches, states):
        rho = node[4]
        a = rng.uniform(0.0, 1.0, (P.na, P.nb, 1))
        qv = rho * rng.uniform(0.0, 0.03, rho.shape) * decay
        qc = rho * rng.uniform(0.0, 3e-3, rho.shape)
        qr = rho * a ** 4 * rng.uniform(0.0, 2e-2, rho.shape)
        tracers.append(np.stack([qv, qc, qr], 0))
        if "ref_tracers" not in P.geom:      # the uniform-diffusion set-up wants them; Kessler never reads them
            P.geom["ref_tracers"] = np.zeros((3, P.na, P.nb, L))
    return g, states, tracers


def kessler_subcycles(grid, states, tracers, dt):
    """Estimate of SUBROUTINE KESSLER's rain sub-cycle count (kessler.f90:113-127) per stored column, in the order of
    stored_columns(), in float64 throughout (the subroutine mixes precisions): it QUALIFIES inputs, it is never compared with a
    kernel."""
    cols = stored_columns(grid)
    out = np.zeros(len(cols), dtype=np.int64)
    for P in grid.patches:
        sel = np.nonzero(cols[:, 0] == P.index)[0]
        i, j = cols[sel, 1], cols[sel, 2]
        rho = states[P.index][0][4][i, j]
        t = tracers[P.index][:, i, j]
        z = np.asarray(P.geom["z_levels"])[i, j]
        rhod = rho - t[0] - t[1] - t[2]
        qr = np.maximum(t[2] / rho, 0.0)
        r = 0.001 * rhod
        vel = 36.34 * (qr * r) ** 0.1364 * np.sqrt(rhod[:, :1] / rhod)
        with np.errstate(divide="ignore"):
            cfl = np.where(vel[:, :-1] != 0.0, 0.8 * (z[:, 1:] - z[:, :-1]) / vel[:, :-1], np.inf)
        dt_max = np.minimum(dt, cfl.min(axis=1))
        out[sel] = np.ceil(dt / dt_max).astype(np.int64)
    return out


def held_suarez_case(L, seed=0):
    """Grid, state and pinned surface pressure for the Held-Suarez kernel at L levels: the baroclinic wave (ne3, 6 patches, 30 km) after
    one oracle ARS343 step of 100 s (W != 0, seam copies consistent, interface-level-0 slots of rho and rho*theta carried along), and
    a surface pressure of 1e5 (1 + 0.01 U(-1,1)) per stored node -- the copies of a seam node get different values."""
    from oracle_lib import Oracle
    g, states = gu.make_grid(3, L, 6, ztop=30000.0)
    o = Oracle(g); o.set_state(0, states)
    assert o.step_ars343(100.0) == 0
    rng = np.random.default_rng(100 + seed)
    ps = [1.0e5 * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, (P.na, P.nb))) for P in g.patches]
    return g, o.get_state(0), ps


def held_suarez_branches(grid, states, ps):
    """The forcing's own formulas (HeldSuarezPhysics.cpp, as orc_held_suarez restates them) in numpy on the interior nodes: sigma of
    the friction loop (pressure from rho * rho*theta, the reference's statement), sigma of the heating loop, and the equilibrium
    temperature before the clamp at 200 K.  ps = None: the tracked interface-level-0 slots."""
    ph = grid.phys
    gamma, kappa = ph.cp / (ph.cp - ph.Rd), ph.Rd / ph.cp
    pscal = ph.p0 * (ph.Rd / ph.p0) ** gamma
    sig_f, sig_h, teq = [], [], []
    for P, (node, edge) in zip(grid.patches, states):
        n = node[:, 1:-1, 1:-1]
        if ps is None:
            surf = pscal * np.exp(np.log(edge[4, 1:-1, 1:-1, 0] * edge[2, 1:-1, 1:-1, 0]) * gamma)
        else:
            surf = ps[P.index][1:-1, 1:-1]
        lat = np.asarray(P.lat)[1:-1, 1:-1, None]
        sig_f.append(pscal * np.exp(np.log(n[4] * n[2]) * gamma) / surf[..., None])
        pr = pscal * np.exp(np.log(n[2]) * gamma)
        sig_h.append(pr / surf[..., None])
        teq.append((315.0 - 60.0 * np.sin(lat) ** 2 - 10.0 * np.log(pr / ph.p0) * np.cos(lat) ** 2) * (pr / ph.p0) ** kappa)
    return np.stack(sig_f), np.stack(sig_h), np.stack(teq)


def lagrange4(xi):
    """Coefficients of the four Lagrange polynomials on the np = 4 GLL nodes at xi; exactly 0 / 1 at a node."""
    c = np.ones(4)
    for m in range(4):
        for n in range(4):
            if n != m:
                c[m] *= (xi - GLL4[n]) / (GLL4[m] - GLL4[n])
    return c


def interp_points(grid, npts, nreta, seed=0):
    """The dict Engine.interp_create / Oracle._interp take: npts sample points on uniformly drawn patches and elements (node_a =
    1 + 4 ea), Lagrange coefficients at xi ~ U(-1,1) -- the first points sit at xi = -1, +1, 0 and on an inner GLL node, so exact 0 / 1
    coefficients occur --, N(0,1) matrices for the conversion to primitive velocities (the kernel takes them as given), and nreta
    operator rows: row 0 a single 1.0 at the top level / top interface, row 1 dense, row 2 all zero, the rest two adjacent weights
    (1 - w, w)."""
    rng = np.random.default_rng(1000 + seed)
    L = grid.L
    patch = rng.integers(0, len(grid.patches), npts)
    node_a = np.zeros(npts, dtype=np.int64); node_b = np.zeros(npts, dtype=np.int64)
    ca = np.zeros((npts, 4)); cb = np.zeros((npts, 4))
    fixed = [(-1.0, 1.0), (1.0, 0.0), (0.0, GLL4[2]), (GLL4[1], -1.0)]
    for i in range(npts):
        P = grid.patches[patch[i]]
        node_a[i] = 1 + 4 * rng.integers(0, (P.na - 2) // 4)
        node_b[i] = 1 + 4 * rng.integers(0, (P.nb - 2) // 4)
        xa, xb = fixed[i] if i < len(fixed) else rng.uniform(-1.0, 1.0, 2)
        ca[i], cb[i] = lagrange4(xa), lagrange4(xb)
    opn = np.zeros((nreta, L)); ope = np.zeros((nreta, L + 1))
    for r in range(nreta):
        if r == 0:
            opn[r, L - 1] = 1.0; ope[r, L] = 1.0
        elif r == 1:
            opn[r] = rng.uniform(0.05, 1.0, L); opn[r] /= opn[r].sum()
            ope[r] = rng.uniform(0.05, 1.0, L + 1); ope[r] /= ope[r].sum()
        elif r == 2:
            pass
        else:
            for op, n in ((opn, L), (ope, L + 1)):
                k = int(rng.integers(0, n - 1)); w = float(rng.uniform(0.05, 0.95))
                op[r, k], op[r, k + 1] = 1.0 - w, w
    return {"patch": patch.astype(np.int32), "node_a": node_a.astype(np.int32), "node_b": node_b.astype(np.int32),
            "coeff_a": ca, "coeff_b": cb, "rll_from_abp": rng.standard_normal((npts, 4)), "op_levels": opn, "op_interfaces": ope}


def interp_state(grid, states, dt=100.0, seed=0):
    """State (and tracers, where the grid has some) to interpolate: the grid's own after one oracle ARS343 step of dt -- the initial
    state has W == 0 and equals the reference state, which turns `state - reference` into 0 / 0 comparisons -- times 1 + 0.01 U(-1,1)
    per entry."""
    from oracle_lib import Oracle
    o = Oracle(grid); o.set_state(0, states)
    nt = int(getattr(grid, "ntracers", 0))
    if nt:
        o.set_tracers(0, [grid.initial_tracers[P.index] for P in grid.patches])
    assert o.step_ars343(dt) == 0
    rng = np.random.default_rng(2000 + seed)
    out = [(n * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, n.shape)), e * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, e.shape))) for n, e in o.get_state(0)]
    tr = [t * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, t.shape)) for t in o.get_tracers(0)] if nt else None
    return out, tr


def interp_longdouble(grid, states, tracers, pts, only_at=0, include_reference_state=True, convert_to_primitive=True, earth_radius=6.37122e6):
    """GridPatchCSGLL::InterpolateData (GridPatchCSGLL.cpp:1644-1760) restated in np.longdouble: per field and source level the 4 x 4
    Lagrange sum over the element, W divided by d_xi R of the element's FIRST node (deriv_r_redge[ia, ib, k, 2], :1665) when
    converting to primitive variables, minus the same sum over the reference state when it is removed, then the operator row; U, V
    through the point's matrix.  Returns (state [5][nreta][npts], tracers [nt][nreta][npts] or None) as longdouble."""
    ld = np.longdouble
    npts, nreta, L = len(pts["patch"]), pts["op_levels"].shape[0], grid.L
    ca, cb = pts["coeff_a"].astype(ld), pts["coeff_b"].astype(ld)
    w2 = ca[:, :, None] * cb[:, None, :]                                   # [npts][4][4]
    opn, ope = pts["op_levels"].astype(ld), pts["op_interfaces"].astype(ld)

    def column(arr_of_patch, comp, extra=None):
        """[npts][nlev]: the horizontal sum at every source level"""
        stacked = np.stack([np.asarray(arr_of_patch(P.index))[comp] for P in grid.patches])      # (every patch has the same box)
        m = np.arange(4)
        x = stacked[pts["patch"][:, None, None], pts["node_a"][:, None, None] + m[None, :, None], pts["node_b"][:, None, None] + m[None, None, :]].astype(ld)
        if extra is not None:
            x = x / extra()[:, None, None, :]
        return np.einsum("imn,imnk->ik", w2, x)

    out = np.zeros((5, nreta, npts), dtype=ld)
    for c in range(5):
        edge = c == 3
        if (only_at == 1 and edge) or (only_at == 2 and not edge):
            continue
        loc = 1 if edge else 0
        dv = None
        if edge and convert_to_primitive:
            dv = lambda: np.stack([np.asarray(grid.patches[p].geom["deriv_r_redge"])[a, b, :, 2] for p, a, b in zip(pts["patch"], pts["node_a"], pts["node_b"])]).astype(ld)
        col = column(lambda p: states[p][loc], c, dv)
        if not include_reference_state:
            col = col - column(lambda p: grid.patches[p].geom["ref_redge" if edge else "ref_node"], c)
        out[c] = (ope if edge else opn) @ col.T
    if convert_to_primitive:
        M = pts["rll_from_abp"].astype(ld)
        ua, ub = out[0] / ld(earth_radius), out[1] / ld(earth_radius)
        out[0], out[1] = M[:, 0] * ua + M[:, 1] * ub, M[:, 2] * ua + M[:, 3] * ub
    tout = None
    if tracers is not None:
        tout = np.stack([opn @ column(lambda p: tracers[p], c).T for c in range(tracers[0].shape[0])])
    return out, tout


def field_distance(got, want, full):
    """max |got - want| per field, relative to max |full| of that field (the field BEFORE the reference state is subtracted); absolute
    where the field is identically zero (W through an operator row that picks the top interface, where W = 0)."""
    out = []
    for c in range(len(want)):
        num, den = gu._pair(got[c], want[c])[0], gu._pair(full[c], full[c])[1]      # inf where a value is not finite; unequal shapes raise
        out.append(float("inf") if float("inf") in (num, den) else num / den if den > 0.0 else num)
    return out


def image_state(grid, states, seed=0):
    """State and tracers for the restart image: the grid's own state times 1 + 0.01 U(-1,1) per entry, W drawn U(-5, 5), the tracers
    the grid's initial ones."""
    rng = np.random.default_rng(3000 + seed)
    out = []
    for n, e in states:
        n = n * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, n.shape)); e = e * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, e.shape))
        e[3] = rng.uniform(-5.0, 5.0, e[3].shape)
        out.append((n, e))
    nt = int(getattr(grid, "ntracers", 0))
    return out, ([np.array(grid.initial_tracers[P.index], copy=True) for P in grid.patches] if nt else None)
