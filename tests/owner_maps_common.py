"""Shared inputs of test_owner_maps_host.py (CPU) and test_gpu_owner_maps.py (GPU): the multi-rank path under the patch-to-rank maps
a caller can hand the engine, first of all the one the reference itself uses.

The reference deals patches to ranks round-robin (Grid::DistributePatches, src/atm/Grid.cpp:1038-1062: m_vecPatchProcessor[n] =
n % nSize), and tmx_define_patch documents owner_rank as that value; Engine(g, rank=r, n_ranks=n) without owner= takes
engine.default_owner, the panel-major block map.  The two differ in what the kernels see: under round-robin nearly every patch edge
has a remote neighbour, nearly every 64-column tile is early, groups of four have their copies on four ranks and cube corners on
three, and rank counts that do not divide the patch count leave ranks with unequal patch counts.

This module imports nothing that needs a GPU: the maps, the case tables, a state whose stored copies all differ (rough_copies), the
co-located nodes found from the grid's coordinates alone (groups_by_position), their mean in long double (mean_longdouble), and the
exchange plan executed in numpy (execute_plan: the arithmetic test_multirank_gloo.py has always checked, shared with it)."""
import ctypes
import numpy as np

import golden_util as gu
from tempestmodel_amd import cubed_sphere
from tempestmodel_amd.engine import Engine, default_owner, reference_owner
from tracer_inputs_common import signed_tracers

# ---------------------------------------------------------------------------------------------
# owner maps: (npatch, n_ranks) -> list of owning ranks


def reference(npatch, n_ranks):
    """Grid::DistributePatches (src/atm/Grid.cpp:1038-1062): patch n goes to rank n % nSize."""
    return reference_owner(npatch, n_ranks)


def block(npatch, n_ranks):
    """engine.default_owner: panel-major blocks."""
    return default_owner(npatch, n_ranks)


def lone_patch(npatch, n_ranks):
    """Rank 0 owns patch 0 alone, the other ranks share the rest in blocks."""
    return [0] + [1 + r for r in default_owner(npatch - 1, n_ranks - 1)]


def shuffled(seed):
    """A fixed permutation of `reference`: the same patch counts per rank, a rank's patches neither contiguous nor strided."""
    def owner(npatch, n_ranks):
        own = np.array(reference(npatch, n_ranks))
        return [int(r) for r in own[np.random.default_rng(seed).permutation(npatch)]]
    return owner


OWNER_MAPS = {"reference": reference, "block": block, "lone_patch": lone_patch, "shuffled": shuffled(5)}


def owner_of(case):
    return OWNER_MAPS[case["map"]](case["npatch"], case["ranks"])


# ---------------------------------------------------------------------------------------------
# case tables


def _case(ne, L, npatch, ntr, ranks, map_, **kw):
    c = dict(ne=ne, L=L, npatch=npatch, ntr=ntr, ranks=ranks, map=map_, case="jw", sw=False)
    c.update(kw)
    return c


def case_id(c):
    return "ne%d-L%d-p%d-t%d-r%d-%s" % (c["ne"], c["L"], c["npatch"], c["ntr"], c["ranks"], c["map"]) + (
        "-sw" if c["sw"] else "") + ("-" + c["case"] if c["case"] != "jw" else "") + ("-" + c["scheme"] if "scheme" in c else "")


# a: the DSS and the pack on their own.  L + 1 (the interface count, the longest slab) on both sides of a multiple of 4, k_dss's level tile.
DSS_CASES = [_case(4, 5, 24, 0, 3, "reference"), _case(4, 3, 24, 5, 2, "reference"), _case(6, 3, 54, 0, 5, "reference"),
             _case(6, 7, 54, 16, 7, "reference"), _case(8, 4, 96, 2, 8, "reference"), _case(2, 3, 24, 1, 2, "lone_patch"),
             _case(4, 6, 24, 0, 4, "shuffled"), _case(12, 3, 24, 0, 5, "block")]

# b: production steps, implicit vertical dynamics; `oracle`: also EXACT against the oracle (ne <= 14)
STEP_CASES = [_case(14, 6, 24, 0, 4, "reference", scheme="ars343", oracle=True),
              _case(14, 6, 24, 0, 3, "reference", scheme="strang", oracle=True),
              _case(12, 6, 24, 0, 4, "reference", scheme="ars343", oracle=True),      # two late tiles
              _case(12, 6, 24, 0, 2, "reference", scheme="ark232", oracle=True),
              _case(18, 3, 54, 0, 5, "reference", scheme="ars343", oracle=False),     # mixed split modes
              _case(14, 6, 24, 0, 4, "shuffled", scheme="ars343", oracle=True)]

# c: the other configurations under `reference`
TRACER_CASE = _case(14, 5, 24, 2, 4, "reference", scheme="ars343")
SUPERCELL_CASE = _case(14, 6, 24, 2, 3, "reference", scheme="strang", case="smallplanet")
SHALLOW_WATER_CASE = _case(14, 1, 24, 0, 3, "reference", scheme="strang", sw=True)
RAYLEIGH_CASE = _case(12, 8, 24, 0, 4, "reference", scheme="ars343", case="schar")
OTHER_CASES = [TRACER_CASE, SUPERCELL_CASE, SHALLOW_WATER_CASE, RAYLEIGH_CASE]

# d: real transport (test_gpu_two_process.py): world, scheme, tracers on ne14 L6, 24 patches
TWO_PROCESS_GRID = (14, 6, 24)
TWO_PROCESS_CASES = [_case(14, 6, 24, 0, 3, "reference", scheme="ars343"), _case(14, 6, 24, 2, 4, "reference", scheme="ars343")]

# what the cases are there for (test_owner_maps_host.py restates each from the plan)
CASE_BOTH_KINDS_OF_TILES = STEP_CASES[0]      # every rank has early and late tiles in both layouts
CASE_TWO_LATE_TILES = STEP_CASES[2]           # a rank with no more than 2 late tiles
CASE_MIXED_SPLIT = STEP_CASES[4]              # element-major: some ranks split, others do not; node-unique tables (2 x 2 tile shape): all have both lists
CASE_FOUR_RANKS_PER_GROUP = DSS_CASES[2]      # four-copy groups on four ranks, all eight cube corners on three
CASE_UNEQUAL_PATCH_COUNTS = DSS_CASES[3]      # 54 patches on 7 ranks: 7 and 8
CASE_LESS_THAN_A_TILE = DSS_CASES[5]          # ne2, 24 patches of one element: rank 0 holds 16 columns

ALL_CASES = DSS_CASES + STEP_CASES + OTHER_CASES + TWO_PROCESS_CASES

_grids = {}


def grid_of(case):
    """(grid, initial states) of a case, built once per process and left unchanged."""
    key = (case["ne"], case["L"], case["npatch"], case["ntr"], case["case"], case["sw"])
    if key not in _grids:
        if case["sw"]:
            ppd = int(round((case["npatch"] / 6) ** 0.5))
            g = cubed_sphere.CubedSphereGrid(case["ne"], 1, 1.0, shallow_water=True, ppd=ppd)
            _grids[key] = (g, g.evaluate_test_case(cubed_sphere.ShallowWaterTest2()))
        else:
            _grids[key] = gu.make_grid(case["ne"], case["L"], case["npatch"], case=case["case"], ntracers=case["ntr"])
    return _grids[key]


# ---------------------------------------------------------------------------------------------
# plan-only engines and what they predict


def plan_engines(grid, owner, n_ranks, **kw):
    return [Engine(grid, device=-2, rank=r, n_ranks=n_ranks, owner=owner, **kw) for r in range(n_ranks)]


def element_major_tiles(e):
    """(early, late) 64-column tiles of a boundary-first stage (tmx_plan_get 7 and 8); (0, 0): the rank does not split."""
    return len(e.plan(7)), len(e.plan(8))


def node_unique_tiles(e, tile_shape=0):
    """(early, late) tiles of the node-unique thread order of a tile shape (tmx_debug_unique_tables what 0, entries 6 and 7; 0 is the
    default shape, the element-major order).  The engine runs a node-unique stage boundary first where both are positive AND the
    element-major lists exist (UniqueLayout::split)."""
    e.lib.tmx_debug_unique_tables.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    sizes = np.zeros(13, dtype=np.int32)
    n = e.lib.tmx_debug_unique_tables(e.h, tile_shape, 0, sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 13)
    assert n >= 8, n
    return int(sizes[6]), int(sizes[7])


def predicted_tiles(case):
    """[(early, late) per rank] of the element-major plan: what tmx_info(TMX_INFO_EARLY_TILES / _LATE_TILES) of the device engines must say."""
    g, _ = grid_of(case)
    kw = dict(fully_explicit=True, uniform_diffusion=(1500.0, 500.0)) if case["case"] == "smallplanet" else {}
    engines = plan_engines(g, owner_of(case), case["ranks"], **kw)
    try:
        return [element_major_tiles(e) for e in engines]
    finally:
        for e in engines:
            e.close()


# ---------------------------------------------------------------------------------------------
# inputs


def rough_copies(states, tracers, seed=41):
    """(states, tracers) in which every STORED copy of a node differs from its co-located copies by an amount of its own magnitude: the
    prognostic slots (U, V, rho*theta, rho on levels) scaled per stored point by uniform(0.5, 2), W on interfaces uniform(-30, 30),
    `tracers` tracers of either sign made as tracer_inputs_common.signed_tracers makes them (from the scaled rho: per stored point as
    well).  A copy taken from the wrong member, the wrong peer or the wrong slab then cannot cancel.  tracers = 0: None."""
    rng = np.random.default_rng(seed)
    out = []
    for node, edge in states:
        node = node.copy(); edge = edge.copy()
        for c in (0, 1, 2, 4):
            node[c] *= rng.uniform(0.5, 2.0, node[c].shape)
        edge[3] = rng.uniform(-30.0, 30.0, edge[3].shape)
        out.append((node, edge))
    return out, (signed_tracers(out, tracers, seed=seed + 1) if tracers else None)


def column_vectors(states, tracers=None):
    """Per patch [na][nb][nv]: the values of a stored column that the exchange carries and the DSS averages, U, V, rho*theta, rho on L
    levels, W on L + 1 interfaces, then every tracer on L levels."""
    out = []
    for p, (n, ed) in enumerate(states):
        parts = [n[0], n[1], n[2], n[4], ed[3]]
        if tracers is not None:
            parts += [t for t in tracers[p]]
        out.append(np.concatenate(parts, axis=-1))
    return out


def scalar_entries(L, ntr):
    """Indices of column_vectors' last axis that hold scalars (everything but U and V)."""
    return np.arange(2 * L, 5 * L + 1 + ntr * L)


# ---------------------------------------------------------------------------------------------
# co-located nodes from the coordinates alone


def groups_by_position(grid):
    """The co-located interior nodes of all patches, from the grid's own coordinates (Patch.X, Patch.Y, panel through
    cubed_sphere.xyz_from_xyp: points of the unit sphere, rounded to 1e-9; the nearest distinct nodes of ne18 are 1e-3 apart) -- nothing
    of tmx_plan_get.  Returns (nodes [N][3] = (patch, i, j) of every interior node, group [N] = index of the node's position among the
    distinct positions, count [positions] = copies stored of it)."""
    nodes, keys = [], []
    for P in grid.patches:
        i, j = np.meshgrid(np.arange(1, P.na - 1), np.arange(1, P.nb - 1), indexing="ij")
        xyz = cubed_sphere.xyz_from_xyp(P.X[i], P.Y[j], P.panel)
        xyz = xyz / np.linalg.norm(xyz, axis=-1, keepdims=True)
        keys.append(np.rint(xyz.reshape(-1, 3) * 1e9).astype(np.int64))
        nodes.append(np.stack([np.full(i.size, P.index), i.ravel(), j.ravel()], 1))
    nodes = np.concatenate(nodes); keys = np.concatenate(keys)
    _, group, count = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
    return nodes, group.ravel(), count


def census_by_owning_ranks(grid, owner, groups=None):
    """{(copies, distinct owning ranks): number of groups} over the groups of two and more copies."""
    nodes, group, count = groups or groups_by_position(grid)
    own = np.asarray(owner)[nodes[:, 0]]
    pairs = np.unique(np.stack([group, own], 1), axis=0)      # one row per (group, owning rank)
    nranks = np.bincount(pairs[:, 0], minlength=len(count))
    out = {}
    for n, r in zip(count, nranks):
        if n >= 2:
            out[(int(n), int(r))] = out.get((int(n), int(r)), 0) + 1
    return out


def gather_nodes(vectors, nodes):
    """[N][nv] values of column_vectors at the nodes of groups_by_position."""
    out = np.empty((len(nodes), vectors[0].shape[-1]))
    for p in np.unique(nodes[:, 0]):
        m = nodes[:, 0] == p
        out[m] = vectors[p][nodes[m, 1], nodes[m, 2]]
    return out


def mean_longdouble(values, group, count):
    """Per position the mean of its copies (values [N][nv]) in numpy.longdouble, and max |copy| per entry: ([positions][nv], [positions][nv])."""
    s = np.zeros((len(count), values.shape[1]), dtype=np.longdouble)
    np.add.at(s, group, values.astype(np.longdouble))
    big = np.zeros((len(count), values.shape[1]))
    np.maximum.at(big, group, np.abs(values))
    return s / count[:, None].astype(np.longdouble), big


# (the bound of the issue, from the kernel's operation order: four copies 0.5 * (0.5 * (a + b) + 0.5 * (c + d)), three roundings; three copies
# (1 / 3) * ((a + b) + c), a rounded 1 / 3, two sums and a product; two copies one rounding)
MEAN_BOUND_ULPS = 4.0


def distance_to_mean(result, inputs, nodes, group, count, entries, panels=None):
    """Worst |result - long double mean of the input copies| over the nodes, in units of 2**-53 * max |copies| of the node and entry, over
    `entries` of the last axis; inf if anything compared is not finite.  panels = the patches' panels: only positions whose copies lie on
    one panel (U and V: the others are rotated before they are averaged).  Positions stored once must come back unchanged."""
    mean, big = mean_longdouble(inputs, group, count)
    keep = np.ones(len(count), dtype=bool)
    if panels is not None:
        pn = np.asarray(panels)[nodes[:, 0]]
        lo = np.full(len(count), 99); hi = np.full(len(count), -1)
        np.minimum.at(lo, group, pn); np.maximum.at(hi, group, pn)
        keep = lo == hi
    sel = keep[group]
    r = result[sel][:, entries]
    if not (np.isfinite(r).all() and np.isfinite(inputs).all()):
        return float("inf")
    d = np.abs(r.astype(np.longdouble) - mean[group[sel]][:, entries])
    unit = big[group[sel]][:, entries] * 2.0 ** -53
    if (d[unit == 0] != 0).any():
        return float("inf")
    single = (count[group[sel]] == 1)
    if (d[single] != 0).any():
        return float("inf")
    return float(np.max(np.where(unit > 0, d / np.where(unit > 0, unit, 1.0), 0.0))) if d.size else 0.0


# ---------------------------------------------------------------------------------------------
# the exchange plan executed in numpy (k_dss's order of operations)


def column_lookup(grid, owner, rank):
    """stored column index -> (patch, i, j) for the rank's patches, the engine's enumeration."""
    np_ = grid.np
    cols = {}
    base = 0
    for P in grid.patches:
        if owner[P.index] != rank:
            continue
        nea = (P.ga1 - P.ga0) // np_; neb = (P.gb1 - P.gb0) // np_
        for a in range(nea):
            for b in range(neb):
                for ii in range(np_):
                    for jj in range(np_):
                        cols[(base + a * neb + b) * 16 + ii * 4 + jj] = (P.index, 1 + a * np_ + ii, 1 + b * np_ + jj)
        base += nea * neb
    return cols


def plan_tables(e):
    """The host plan of an engine (plan-only ones too) as execute_plan takes it."""
    return dict(NS=int(e.plan(3)[0]), send=e.plan(0).reshape(-1, 4), recv=e.plan(1).reshape(-1, 4), grp=e.plan(2).reshape(-1, 5),
                gx=e.plan(4), gt=e.plan(5), M=e.plan_matrices())


def execute_plan(tab, cols, L, column_values, ghost):
    """The averaging of every DSS group of a rank exactly as k_dss does it.  tab: plan_tables; cols: column_lookup; column_values(p, i, j):
    the stored column as column_vectors orders it; ghost [n_recv][nv]: the received columns in ghost-buffer order.  Yields
    ((patch, i, j), averaged column) for every LOCAL member of every group."""
    NS, grp, gx, gt, M = tab["NS"], tab["grp"], tab["gx"], tab["gt"], tab["M"]
    for gi, row in enumerate(grp):
        n = row[0]; mem = row[1:1 + n]
        vals = np.array([column_values(*cols[c]) if c < NS else ghost[c - NS] for c in mem])
        ty = [(int(gt[gi]) >> (2 * m)) & 3 for m in range(4)]

        def comb(v, m):
            # k_dss / GridCSGLL::ApplyDSS order of operations (see tmx_host.hip, "device group tables")
            if n == 2:
                return 0.5 * (v[0] + v[1])
            if n == 4:
                pr = {0: ((0, 1), (2, 3)), 1: ((0, 2), (1, 3)), 2: ((0, 3), (1, 2))}[ty[m]]
                return 0.5 * (0.5 * (v[pr[0][0]] + v[pr[0][1]]) + 0.5 * (v[pr[1][0]] + v[pr[1][1]]))
            nx, pv = (m + 1) % 3, (m + 2) % 3
            f, s2 = (pv, nx) if ty[m] else (nx, pv)
            return (1.0 / 3.0) * ((v[m] + v[f]) + v[s2])
        res = np.array([comb(vals, m) for m in range(n)])
        if gx[gi] >= 0:
            T = M[gx[gi]]
            ua = vals[:, 0:L]; ub = vals[:, L:2 * L]
            for m in range(n):
                fa = np.array([ua[q] if q == m else T[m, q, 0, 0] * ua[q] + T[m, q, 0, 1] * ub[q] for q in range(n)])
                fb = np.array([ub[q] if q == m else T[m, q, 1, 0] * ua[q] + T[m, q, 1, 1] * ub[q] for q in range(n)])
                res[m, 0:L] = comb(fa, m)
                res[m, L:2 * L] = comb(fb, m)
        for m, c in enumerate(mem):
            if c < NS:
                yield cols[c], res[m]
