"""Tables, inputs and oracle results of tests/test_gpu_scheme_matrix.py: all ten time schemes in every configuration that changes what
tmx_step runs on the device.  tests/test_schemes_inputs_host.py qualifies them on the C oracle and on the library's host logic alone,
without a device.

A CELL is (configuration, scheme).  It runs SEQUENCE -- first step, two plain steps, a step with the last-step flag, and one more first
step: a run restarted on the same engine -- from the configuration's own initial state, and after every step compares instance 0 (state
and tracers) and, for the five Strang schemes, the carried instance 1 (which the last step leaves without the closing combination,
TimestepSchemeStrang.cpp:654-657).

    name            grid / options                                       dt     what it selects on the device
    jw              make_grid(3, 5, 6)                                   100    node-unique interpreter, stored prefix, column solve on unique columns
    jw_tr           the same with two tracers of any sign                100    element-major; implicit tracer column update; both negative-tracer
                                                                                filters; Strang's vertical filter on every step that is not a first one
    schar           Schar mountain, L6                                   0.5    topography, Rayleigh layer, "unique_mixed"; Strang stays element-major
    expl            small planet, L6, fully explicit vertical mode       1.0    V.StepImplicit a no-op in the access analysis; ARK232's terms kernel in
                                                                                the explicit mode
    expl_udiff_tr   the same with uniform diffusion and two tracers      1.0    the supercell configuration under every scheme
    visc2, visc0    jw with one viscosity pass / nu = 0                  100    one-pass and inactive StepAfterSubCycle (other sharing decisions)
    sw              shallow water, ne4, perturbed Williamson test 2      200    k_sw_explicit under every scheme; ARK232's terms call is the stub's no-op
    jw_p24, jw_tr_p24   jw and jw_tr on ne10 / 24 patches                100    three rank engines: the smallest 24-patch grid on which every rank of
                                                                                three owns early and late tiles (5 x 5 elements per patch)

Which interpreter runs a step (expect_unique): the node-unique one where the configuration is eligible (no tracers, implicit vertical
dynamics, no uniform diffusion, not shallow water, no graph replay) and the option is on, EXCEPT by design
    * the Strang family with a Rayleigh layer (schar): the closing column solve of the relaxed state has no node-unique form
      (tmx_debug_program_rayleigh == 0): element-major, every step;
    * ARK232 on a grid where the in-patch copies of some node differ in a bit of the per-column geometry StepImplicitTermsExplicitly reads
      (vite_copies_agree false; the reference evaluates that operator per stored copy): element-major, every step;
    * ARS232 / ARS443 with a Rayleigh layer: their programs cannot read the relaxed (element-major) model state copy by copy
      (tmx_debug_program_mixed == 0), so every step checks its copies on the device and runs node-unique or element-major by what it finds:
      data-dependent, the interpreter is not asserted there (the results are).
The first step of a cell starts from a pointwise state whose seam copies may differ: which interpreter it takes is asserted only where it
is structural (the schemes that read the model state copy by copy)."""
import ctypes
import functools
import numpy as np
import golden_util as gu
import tracer_inputs_common as tc
from parity_common import UDIFF

SCHEMES = ["ars343", "ars232", "ars222", "ars443", "ark232", "strang", "strang_fe", "strang_rk4", "strang_ssp3", "strang_ssprk53"]
STRANG = [s for s in SCHEMES if s.startswith("strang")]
NINST = 10
SEQUENCE = [(True, False), (False, False), (False, False), (False, True), (True, False)]      # (first, last) of every step of a cell
NU2 = (2.0e5, 2.0e5, 2.0e5)
CONFIGS = ["jw", "jw_tr", "schar", "expl", "expl_udiff_tr", "visc2", "visc0", "sw"]
UNIQUE_CONFIGS = ["jw", "schar", "visc2", "visc0"]      # eligible for the node-unique layout: run with "unique_layout" 1 and 0
RANK_CONFIGS = ["jw_p24", "jw_tr_p24"]
N_RANKS, RANKS_NE = 3, 10
GRAPH_CONFIGS = ["jw", "expl_udiff_tr"]
# one engine, one oracle, one program after the other: a program starts from the slot sharing and the forms another one left behind
MIXED_SEQUENCE = [("ars343", False, False), ("strang", True, False), ("strang", False, False), ("ark232", False, False), ("ars443", False, False),
                  ("strang_rk4", True, False), ("strang_rk4", False, True), ("ars222", False, False), ("strang_ssprk53", True, False)]
MIXED_CONFIGS = ["jw", "jw_tr", "expl_udiff_tr"]


def _sw_case():
    """Williamson test 2 at ne4 is a steady state and hardly moves: the height gets a smooth wave-2 pattern of 2 %, the wind a smooth
    factor within 15 % of one (a scalar times the vector: the panels' components stay one field)."""
    from tempestmodel_amd.cubed_sphere import CubedSphereGrid, ShallowWaterTest2
    g = CubedSphereGrid(4, 1, 1.0, shallow_water=True)
    states = g.evaluate_test_case(ShallowWaterTest2())
    out = []
    for P, (n, e_) in zip(g.patches, states):
        n = n.copy()
        lon, lat = np.asarray(P.lon), np.asarray(P.lat)
        f = 1.0 + 0.3 * np.cos(lat) * np.sin(lat) * np.cos(lon + 0.4)
        n[0, ..., 0] *= f; n[1, ..., 0] *= f
        n[2, ..., 0] *= 1.0 + 0.02 * np.cos(lat) ** 2 * np.sin(2.0 * lon + 0.5)
        out.append((n, e_))
    return g, out


@functools.lru_cache(maxsize=None)
def config(name):
    """(grid, initial state, tracers or None, keywords of Engine and Oracle alike, dt).  Cached and shared: handed out read-only, and no
    caller modifies the grid."""
    if name in ("jw", "visc2", "visc0"):
        g, st = _jw_grid()
        kw = {"visc2": dict(hypervis_order=2, nu=NU2), "visc0": dict(nu=(0.0, 0.0, 0.0))}.get(name, {})
        return g, st, None, kw, 100.0
    if name == "jw_tr":
        g, st, _, tr, _ = tc.case(5, 2)
        return g, st, tr, {}, 100.0
    if name == "schar":
        g, st = gu.make_grid(3, 6, 6, case="schar")
        return g, tc._ro(st), None, {}, 0.5
    if name == "expl":
        g, st = gu.make_grid(3, 6, 6, case="smallplanet")
        return g, tc._ro(st), None, dict(fully_explicit=True), 1.0
    if name == "expl_udiff_tr":
        g, st, _, tr, _ = tc.case(6, 2, name="smallplanet")
        return g, st, tr, dict(fully_explicit=True, uniform_diffusion=UDIFF), 1.0
    if name == "sw":
        g, st = _sw_case()
        return g, tc._ro(st), None, {}, 200.0
    if name == "jw_p24":
        g, st = gu.make_grid(RANKS_NE, 5, 24)
        return g, tc._ro(st), None, {}, 100.0
    if name == "jw_tr_p24":
        g, st, _, tr, _ = tc.case(5, 2, ne=RANKS_NE, npatch=24)
        return g, st, tr, {}, 100.0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _jw_grid():
    g, st = gu.make_grid(3, 5, 6)
    return g, tc._ro(st)


def new_oracle(name):
    from oracle_lib import Oracle
    g, st, tr, kw, _ = config(name)
    o = Oracle(g, ninst=NINST, **kw)
    o.set_state(0, st)
    if tr is not None:
        o.set_tracers(0, tr)
    return o


def snapshot(o, ix):
    return tc._ro((o.get_state(ix), o.get_tracers(ix) if o.ntracers else None))


def compared_instances(scheme):
    return (0, 1) if scheme in STRANG else (0,)


@functools.lru_cache(maxsize=None)
def want(name, scheme, flag=True):
    """What the oracle leaves after every step of SEQUENCE: [{instance: (state, tracers or None)}] with instances 0 and 1 (the host file
    looks at both for every scheme, the GPU file at compared_instances), and the oracle's return codes.  ``flag`` False: the same
    run with the last-step flag never set."""
    o = new_oracle(name)
    dt = config(name)[4]
    snaps, rcs = [], []
    for first, last in SEQUENCE:
        rcs.append(o.step(scheme, dt, first=first, last=last and flag))
        snaps.append({ix: snapshot(o, ix) for ix in (0, 1)})
    return snaps, rcs


@functools.lru_cache(maxsize=None)
def want_mixed(name):
    """The same after every step of MIXED_SEQUENCE on one oracle."""
    o = new_oracle(name)
    dt = config(name)[4]
    snaps, rcs = [], []
    for scheme, first, last in MIXED_SEQUENCE:
        rcs.append(o.step(scheme, dt, first=first, last=last))
        snaps.append({ix: snapshot(o, ix) for ix in (0, 1)})
    return snaps, rcs


def finite(snap):
    """every compared entry (prognostic slots and tracers on interior nodes) is finite"""
    st, tr = snap
    return max(gu.prognostic_errors(st, st)) == 0.0 and (tr is None or max(gu.tracer_errors(tr, tr)) == 0.0)


def differences(a, b, shallow_water=False):
    """The error figures of snapshot a against b, one per compared variable (U, V, rho*theta or h, W, rho -- the first three with the
    shallow-water set --, then the tracers)."""
    errs = gu.prognostic_errors(a[0], b[0])
    errs = errs[:3] if shallow_water else errs
    return list(errs) + (list(gu.tracer_errors(a[1], b[1])) if a[1] is not None else [])


# ------------------------------------------------------------------------------------------------------------------------------
# which interpreter a step runs: the library's host logic (tmx_debug_*: no device) and the grid's arrays

def _lib():
    from tempestmodel_amd.engine import load_library
    lib = load_library()
    lib.tmx_debug_program_prefix.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)] * 2 + [ctypes.c_int]
    return lib


def scheme_id(scheme):
    from tempestmodel_amd.engine import Engine
    return Engine.SCHEMES[scheme]


def has_unique_form(scheme, first, last):
    return _lib().tmx_debug_program_unique(scheme_id(scheme), int(first), int(last)) > 0


def reads_copy_by_copy(scheme, first, last):
    return _lib().tmx_debug_program_mixed(scheme_id(scheme), int(first), int(last), 0) == 1


def keeps_unique_with_rayleigh(scheme, first, last):
    return _lib().tmx_debug_program_rayleigh(scheme_id(scheme), int(first), int(last)) == 1


def prefix_pairs(scheme, first, last):
    return _lib().tmx_debug_program_prefix(scheme_id(scheme), int(first), int(last), None, None, 0)


@functools.lru_cache(maxsize=None)
def vite_copies_agree(name):
    """UniqueLayout::vite_ok restated on the grid's arrays (tmx_unique.hip, tmxu_build): do the in-patch copies of every node -- the last
    node of an element and the first of the next, along either direction -- carry the same bits in the per-column geometry
    k_vi_terms_explicit reads: the 2-D contravariant metric, the Jacobians on the lowest level and interface, d_xi R, the cube coordinates
    and the topography derivatives the closed-form 3-D metric is made of?"""
    return grid_copies_agree(config(name)[0])


def grid_copies_agree(g):
    for P in g.patches:
        ge = P.geom
        na, nb = P.na, P.nb
        X = np.broadcast_to(np.asarray(P.X, dtype=np.float64)[:, None], (na, nb))
        Y = np.broadcast_to(np.asarray(P.Y, dtype=np.float64)[None, :], (na, nb))
        fields = [np.asarray(ge["contra_metric_2d_a"])[..., 0], np.asarray(ge["contra_metric_2d_a"])[..., 1], np.asarray(ge["contra_metric_2d_b"])[..., 1],
                  np.asarray(ge["jacobian"])[..., 0], np.asarray(ge["jacobian_redge"])[..., 0], np.asarray(ge["deriv_r_node"])[..., 0, 2], X, Y,
                  np.asarray(ge["topography_deriv"])[..., 0], np.asarray(ge["topography_deriv"])[..., 1]]
        for f in fields:
            f = f.reshape(na, nb)[1:-1, 1:-1]
            for i in range(3, na - 2 - 1, 4):
                if not np.array_equal(f[i], f[i + 1]):
                    return False
            for j in range(3, nb - 2 - 1, 4):
                if not np.array_equal(f[:, j], f[:, j + 1]):
                    return False
    return True


def expect_unique(name, scheme, first, last):
    """True / False: a step of this program, not the first of a cell, runs on the node-unique / the element-major layout (option on);
    None: decided by the data (the module's header)."""
    if name not in UNIQUE_CONFIGS or not has_unique_form(scheme, first, last):
        return False
    if scheme == "ark232" and not vite_copies_agree(name):
        return False
    if name == "schar":
        if not keeps_unique_with_rayleigh(scheme, first, last):
            return False
        if not reads_copy_by_copy(scheme, first, last):
            return None
    return True


def expect_mixed_steps(name, scheme, k):
    """TMX_INFO_MIXED_STEPS after step k + 1 of a cell (option on): the steps so far whose explicit stages read an element-major model
    state copy by copy.  Without a Rayleigh layer that is the first step alone (the uploaded state); with one, every step (the
    relaxation at the end of StepAfterSubCycle leaves the model state element-major)."""
    first, last = SEQUENCE[k]
    if expect_unique(name, scheme, first, last) is not True or not reads_copy_by_copy(scheme, first, last):
        return 0
    return k + 1 if name == "schar" else 1
