"""Inputs and oracle results of tests/test_gpu_tracer_transport_shapes.py: tracer fields of any sign on which both positive-definite
filters (HorizontalDynamicsFEM::FilterNegativeTracers per element and level, VerticalDynamicsFEM::FilterNegativeTracers per column)
act in every one of their cases, at one to sixteen tracers.  tests/test_tracer_inputs_host.py qualifies them on the C oracle and in
numpy alone, without a device.

Both filters compute r = total / nonneg (total: the area-weighted sum over the element's 16 nodes or the column's L levels; nonneg:
the same sum over the entries q >= 0) and store (q > 0) ? q * r : 0.  The cases, named by the input of one element or column:

    mixed       entries of both signs, net mass positive: negatives clipped, r in (0, 1)
    net < 0     entries of both signs, net mass negative: r < 0, the positive entries come out NEGATIVE
    all <= 0    nothing positive, something negative: r = total / (-0.0 or 0.0) = -inf (or +inf), never multiplied: all +0.0
    all zero    r = 0 / 0 = NaN, never multiplied: all +0.0

Tracer c is rho * m_c with m_c = 1e-3 |1 + 0.3 N(0, 1)| per node from a seeded generator (the issue's recipe reads 1e-3 (1 + 0.3 N(0, 1));
the absolute value is this file's one departure from it: a draw below -3.3 sigma would otherwise put a negative node into the fields
that "positive" names, kind 3 among them), then by kind c % 4:

    kind 0      the sign flipped at 30 % of the nodes
    kind 1      per (element, level) one of {all negative, all exactly zero, positive, positive}, drawn uniformly
    kind 2      per stored column one of {all negative, all zero, alternating +1, -0.5 by level, positive}, drawn uniformly
    kind 3      positive

Kinds 0 and 1 carry the horizontal filter's cases, kinds 0 and 2 the vertical filter's."""
import functools
import numpy as np
import golden_util as gu
from parity_common import UDIFF

NP = 4      # nodes per element edge
SHAPES = [(3, 1), (4, 5), (5, 4), (7, 16), (30, 3)]      # (levels, tracers) on ne3 / 6 patches
SHAPES_UDIFF = [(3, 4), (5, 5)]
SHAPES_STEPS = [(7, 4), (7, 16)]
SHAPE_VISC = (5, 4)
SHAPE_RANKS = (5, 4)      # on ne12 / 24 patches
DT = 100.0                # the baroclinic wave on ne3 / ne12
DT_UDIFF = 0.7            # the small planet
NINST = 10                # instances of every oracle and engine here (ARK232 and Strang take more than ARS343's seven)
DT_SCHAR = 0.5            # the Schar mountain's reduced sphere (levels_common: 100 s does not stay finite there)
NU2 = (2.0e5, 2.0e5, 2.0e5)
COMBINE = [0.5, -1.25, 0.75, 1.0, 0.0, 0.0, 0.0]      # instance 5 <- 0.5 x input - 1.25 x H.StepExplicit + 0.75 x V.StepImplicit + StepAfterSubCycle


def signed_tracers(states, nt, seed=23):
    """The recipe of the module's header on the rho of ``states``: [nt][na][nb][L] per patch, halo ring included (kind 1 leaves it
    positive: it belongs to no element of the patch)."""
    rng = np.random.default_rng(seed)
    out = []
    for node, _ in states:
        rho = node[4]
        na, nb, L = rho.shape
        nea, neb = (na - 2) // NP, (nb - 2) // NP
        t = np.empty((nt,) + rho.shape)
        for c in range(nt):
            q = rho * 1e-3 * np.abs(1.0 + 0.3 * rng.standard_normal(rho.shape))
            kind = c % 4
            if kind == 0:
                q = np.where(rng.uniform(size=rho.shape) < 0.3, -q, q)
            elif kind == 1:
                draw = rng.integers(0, 4, (nea, neb, L))
                f = np.ones(rho.shape)
                f[1:-1, 1:-1] = np.repeat(np.repeat(np.select([draw == 0, draw == 1], [-1.0, 0.0], 1.0), NP, 0), NP, 1)
                q = q * f
            elif kind == 2:
                draw = rng.integers(0, 4, (na, nb))[..., None]
                alt = np.where(np.arange(L) % 2 == 0, 1.0, -0.5)
                q = q * np.select([draw == 0, draw == 1, draw == 2], [-1.0, 0.0, alt[None, None, :]], 1.0)
            t[c] = q
        t += 0.0      # no -0.0 from the products by zero: the recipe's zeros are +0.0 (negative_zeros plants the others)
        out.append(t)
    return out


def negative_zeros(tracers, seed=29, per_tracer=5):
    """Copies with -0.0 planted in per_tracer interior entries of every tracer and patch; returns (tracers, [index arrays])."""
    rng = np.random.default_rng(seed)
    out, where = [], []
    for t in tracers:
        t = t.copy()
        nt, na, nb, L = t.shape
        ix = np.stack([np.repeat(np.arange(nt), per_tracer), rng.integers(1, na - 1, nt * per_tracer),
                       rng.integers(1, nb - 1, nt * per_tracer), rng.integers(0, L, nt * per_tracer)], 0)
        t[tuple(ix)] = -0.0
        out.append(t); where.append(ix)
    return out, where


def rough_state(states, seed=5):
    """The rough state of test_gpu_tracer_column_shapes._case: U, V + uniform(-20, 20), rho*theta and rho x (1 + 0.01 N(0, 1)), W on
    interfaces uniform(-3, 3) -- the tracer fluxes change sign from node to node."""
    rng = np.random.default_rng(seed)
    out = []
    for n, e_ in states:
        n = n.copy(); e_ = e_.copy()
        n[0] += rng.uniform(-20.0, 20.0, n[0].shape); n[1] += rng.uniform(-20.0, 20.0, n[1].shape)
        n[2] *= 1.0 + 0.01 * rng.standard_normal(n[2].shape); n[4] *= 1.0 + 0.01 * rng.standard_normal(n[4].shape)
        e_[3] = rng.uniform(-3.0, 3.0, e_[3].shape)
        out.append((n, e_))
    return out


@functools.lru_cache(maxsize=None)
def case(L, nt, ne=3, npatch=6, name="jw", reference_length=None):
    """(grid, the case's own state, rough state, tracers, scrub tracers).  With the small planet the reference columns of the uniform
    diffusion are set: the smooth state and 0.9 |tracers|.  ``reference_length``: written to the grid before anything is built from
    it.  The Schar mountain defines no tracers of its own: the grid is told their number.
    The result is cached and shared by every test of the process: states and tracers are handed out read-only, and the grid must not
    be modified by a caller (whatever a case needs written to it is written here, before the first use)."""
    g, st = gu.make_grid(ne, L, npatch, case=name, ntracers=nt)
    if getattr(g, "ntracers", 0) != nt:
        g.ntracers = nt
    if reference_length is not None:
        g.reference_length = reference_length
    tr = signed_tracers(st, nt)
    if name == "smallplanet":
        for P, (n, e_), t in zip(g.patches, st, tr):
            P.geom["ref_node"] = n.copy(); P.geom["ref_redge"] = e_.copy(); P.geom["ref_tracers"] = 0.9 * np.abs(t)
    return g, _ro(st), _ro(rough_state(st)), _ro(tr), _ro(signed_tracers(st, nt, seed=31))


# ------------------------------------------------------------------------------------------------------------------------------
# the plain restatement of both filters


def filter_h_numpy(grid, tracers):
    """HorizontalDynamicsFEM::FilterNegativeTracers restated: the sums run over i then j in a Python loop, everything else (element,
    level, tracer) is vectorised.  ``np.where`` never forms q * r where q <= 0."""
    out = []
    for P, t in zip(grid.patches, tracers):
        t = t.copy()
        nt, na, nb, L = t.shape
        nea, neb = (na - 2) // NP, (nb - 2) // NP
        q = t[:, 1:-1, 1:-1].reshape(nt, nea, NP, neb, NP, L)      # [c][a][i][b][j][k]
        area = P.geom["element_area_node"][1:-1, 1:-1].reshape(nea, NP, neb, NP, L)
        total = np.zeros((nt, nea, neb, L)); nonneg = np.zeros((nt, nea, neb, L))
        for i in range(NP):
            for j in range(NP):
                pm = q[:, :, i, :, j] * area[None, :, i, :, j]
                total = total + pm
                nonneg = np.where(q[:, :, i, :, j] >= 0.0, nonneg + pm, nonneg)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = total / nonneg
            res = np.where(q > 0.0, q * r[:, :, None, :, None, :], 0.0)
        t[:, 1:-1, 1:-1] = res.reshape(nt, na - 2, nb - 2, L)
        out.append(t)
    return out


def filter_v_numpy(grid, tracers):
    """VerticalDynamicsFEM::FilterNegativeTracers restated: the sums run over k ascending in a Python loop."""
    out = []
    for P, t in zip(grid.patches, tracers):
        t = t.copy()
        q = t[:, 1:-1, 1:-1]
        area = P.geom["element_area_node"][1:-1, 1:-1]
        total = np.zeros(q.shape[:-1]); nonneg = np.zeros(q.shape[:-1])
        for k in range(q.shape[-1]):
            pm = q[..., k] * area[None, ..., k]
            total = total + pm
            nonneg = np.where(q[..., k] >= 0.0, nonneg + pm, nonneg)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = total / nonneg
            res = np.where(q > 0.0, q * r[..., None], 0.0)
        t[:, 1:-1, 1:-1] = res
        out.append(t)
    return out


def cells(t, vertical):
    """One patch's interior tracer values grouped by the filter's unit: [units][members] -- per (tracer, element, level) the 16 nodes,
    or per (tracer, column) the L levels."""
    nt, na, nb, L = t.shape
    q = t[:, 1:-1, 1:-1]
    if vertical:
        return q.reshape(-1, L)
    nea, neb = (na - 2) // NP, (nb - 2) // NP
    return q.reshape(nt, nea, NP, neb, NP, L).transpose(0, 1, 3, 5, 2, 4).reshape(-1, NP * NP)


def cells_of_tracers(t, vertical, keep):
    """cells() of the tracers whose kind (c % 4) is in ``keep``."""
    sel = [c for c in range(t.shape[0]) if c % 4 in keep]
    return cells(t[sel], vertical)


CLASSES = ("r != 1", "0 < r < 1", "net < 0", "all <= 0", "all zero")


def class_masks(cin):
    """Input masks of the four cases over cells() of the INPUT: by construction, from the input alone."""
    pos, neg = (cin > 0.0).any(1), (cin < 0.0).any(1)
    return {"all <= 0": ~pos & neg, "all zero": ~pos & ~neg, "has positive": pos}


def class_counts(cin, cout):
    """How many units of each case one patch holds, counted as the issue states them: on the filter's OUTPUT where it says "left" /
    "holding", on the input where it names the input.  "r != 1": units holding zeros and non-zeros whose r is not 1 -- the issue's
    first condition, which takes in the units of net negative mass; "0 < r < 1": those of them that hold no negative value, the
    header's "mixed" case proper."""
    m = class_masks(cin)
    zeros, nonzero, negative = (cout == 0.0).any(1), (cout != 0.0).any(1), (cout < 0.0).any(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(cin > 0.0, cout / cin, np.nan)
    r_not_1 = np.nanmax(np.abs(np.where(np.isnan(ratio), 1.0, ratio) - 1.0), 1) > 0.0
    return {"r != 1": int((zeros & nonzero & r_not_1).sum()),
            "0 < r < 1": int((zeros & nonzero & r_not_1 & ~negative).sum()),
            "net < 0": int(negative.sum()),
            "all <= 0": int(m["all <= 0"].sum()),
            "all zero": int(m["all zero"].sum())}


# ------------------------------------------------------------------------------------------------------------------------------
# what the oracle leaves: computed once per shape, shared by the host and the GPU file, never changed by either


def _ro(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, (list, tuple)):
        for y in x:
            _ro(y)
    return x


def snapshot(o, ix):
    return _ro((o.get_state(ix), o.get_tracers(ix)))


def oracle(g, **kw):
    from oracle_lib import Oracle
    return Oracle(g, ninst=NINST, **kw)


@functools.lru_cache(maxsize=None)
def want_percall(L, nt, which, dt=DT):
    """(a) and, with dt = 0.0, (b): instance 0 the input (``which``: "rough" or "smooth" state), 1 H.StepExplicit(0, 1), 2 V.StepImplicit
    in place on a copy (L >= 4: the header of test_gpu_tracer_column_shapes.py), 3 and 4 StepAfterSubCycle(0, 3, 4), 5 the combination
    COMBINE of 0 to 3.  {instance: (state, tracers)}"""
    g, st, rough, tr, _ = case(L, nt)
    o = oracle(g)
    o.set_state(0, rough if which == "rough" else st); o.set_tracers(0, tr)
    o.copy_data(0, 1); o.h_step_explicit(0, 1, dt)
    o.copy_data(0, 2)
    if L >= 4 and dt != 0.0:
        assert o.v_step_implicit(2, 2, dt) == 0
    o.h_step_after_subcycle(0, 3, 4, dt)
    o.copy_data(0, 5); o.linear_combine_data(COMBINE, 5)
    return {ix: snapshot(o, ix) for ix in range(6)}


@functools.lru_cache(maxsize=None)
def want_filters(L, nt, vertical, plant=False):
    """The oracle's exported filter applied to the input tracers themselves (``plant``: with negative_zeros first):
    (input tracers, filtered tracers, planted indices or None)"""
    g, st, _, tr, _ = case(L, nt)
    where = None
    if plant:
        tr, where = negative_zeros(tr)
    o = oracle(g)
    o.set_state(0, st); o.set_tracers(0, tr)
    (o.filter_negative_tracers_v if vertical else o.filter_negative_tracers_h)(0)
    return _ro(tr), _ro(o.get_tracers(0)), where


VISC = {"order2": dict(nu=NU2, hypervis_order=2), "order0": dict(hypervis_order=0), "nu0": dict(nu=(0.0, 0.0, 0.0), hypervis_order=4),
        "reflen0": dict(hypervis_order=4)}


def visc_case(key):
    """(case(...), engine / oracle keywords, dt) of (d): the four configurations at SHAPE_VISC, the Schar mountain at orders 2 and 0."""
    if key.startswith("schar_"):
        return case(6, 2, name="schar"), VISC[key[6:]], DT_SCHAR
    return case(*SHAPE_VISC, reference_length=0.0 if key == "reflen0" else None), VISC[key], DT


VISC_KEYS = ["order2", "order0", "nu0", "reflen0", "schar_order2", "schar_order0"]


@functools.lru_cache(maxsize=None)
def want_visc(key):
    """(d): StepAfterSubCycle(0, 3, 4) per call on the rough state (the case's own is the Schar mountain's reference state, which the
    Rayleigh layer leaves alone), then two ARS343 steps from the case's state: (instance 3, instance 4, [step 1, 2])"""
    (g, st, rough, tr, _), kw, dt = visc_case(key)
    o = oracle(g, **kw)
    o.set_state(0, rough); o.set_tracers(0, tr)
    o.h_step_after_subcycle(0, 3, 4, dt)
    call = (snapshot(o, 3), snapshot(o, 4))
    o.set_state(0, st); o.set_tracers(0, tr)
    steps = []
    for _ in range(2):
        assert o.step_ars343(dt) == 0
        steps.append(snapshot(o, 0))
    return call + (steps,)


@functools.lru_cache(maxsize=None)
def want_udiff(L, nt):
    """(e): the small planet, fully explicit, uniform diffusion, rough state: H.StepExplicit, V.StepExplicit, StepImplicitTermsExplicitly
    each on a copy of instance 0 (-> 1, 2, 3); then from the case's state two ARS343 and two Strang steps.  (calls, steps)"""
    g, st, rough, tr, _ = case(L, nt, name="smallplanet")
    o = oracle(g, fully_explicit=True, uniform_diffusion=UDIFF)
    o.set_state(0, rough); o.set_tracers(0, tr)
    calls = []
    for ix, name in ((1, "h_step_explicit"), (2, "v_step_explicit"), (3, "v_step_implicit_terms_explicitly")):
        o.copy_data(0, ix)
        getattr(o, name)(0, ix, DT_UDIFF)
        calls.append((name, snapshot(o, ix)))
    o.set_state(0, st); o.set_tracers(0, tr)
    steps = []
    for scheme, first in (("ars343", True), ("ars343", False), ("strang", True), ("strang", False)):
        assert o.step(scheme, DT_UDIFF, first=first) == 0
        steps.append((scheme, first, snapshot(o, 0)))
    return calls, steps


STEP_PROGRAMS = {"ars343": [("ars343", True), ("ars343", False)], "strang": [("strang", True), ("strang", False)],
                 "ark232": [("ark232", True), ("ark232", False)]}


_STEPPING = {}      # (L, nt, program, ne, npatch) -> (oracle, snapshots so far)


def want_step(L, nt, program, k, ne=3, npatch=6):
    """(f), (g): (state, tracers) after step k + 1 of STEP_PROGRAMS[program] from the case's state; Strang's second step is
    LinearCombine + the vertical filter on its own.  The oracle advances only as far as it is asked, so each case of a test that is
    split by step pays for its own step."""
    key = (L, nt, program, ne, npatch)
    if key not in _STEPPING:
        g, st, _, tr, _ = case(L, nt, ne=ne, npatch=npatch)
        o = oracle(g)
        o.set_state(0, st); o.set_tracers(0, tr)
        _STEPPING[key] = (o, [])
    o, snaps = _STEPPING[key]
    while len(snaps) <= k:
        scheme, first = STEP_PROGRAMS[program][len(snaps)]
        assert o.step(scheme, DT, first=first) == 0
        snaps.append(snapshot(o, 0))
    return snaps[k]


def want_steps(L, nt, program, ne=3, npatch=6):
    """[(state, tracers) after each step] of the whole program"""
    return [want_step(L, nt, program, k, ne=ne, npatch=npatch) for k in range(len(STEP_PROGRAMS[program]))]


def interior_finite(snap):
    (states, tracers) = snap
    return (all(np.isfinite(n[:, 1:-1, 1:-1]).all() and np.isfinite(e[:, 1:-1, 1:-1]).all() for n, e in states)
            and all(np.isfinite(t[:, 1:-1, 1:-1]).all() for t in tracers))


def fractions(tracers):
    """(share of exact zeros, share of negative values) over the interior of all patches"""
    q = np.concatenate([t[:, 1:-1, 1:-1].ravel() for t in tracers])
    return float(np.mean(q == 0.0)), float(np.mean(q < 0.0))
