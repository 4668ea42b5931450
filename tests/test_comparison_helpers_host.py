"""The comparison helpers of the parity tests (golden_util.prognostic_errors / tracer_errors / interp_rel, parity_common._cmp, the
wrappers of test_gpu_stage_walk_segments.py and test_gpu_dcmip_physics.py, levels_common.field_distance) judged on synthetic states:
no engine, no library.  About 170 comparisons of the suite go through them, and they used to take their maxima with Python's max(),
for which max(0.0, nan) == 0.0: a NaN in the device's result compared as an exact match.

The toy layout is three patches of node[5][6][6][3], redge[5][6][6][4] and tracers[2][6][6][3] (a 4 x 4 interior inside a halo ring).
What is asserted:
  * a NaN, +inf or -inf planted in a compared slot -- each prognostic variable and each tracer, in the first, middle or last patch, on
    the device's side, the reference's, or the same value on both -- makes that variable's error inf, which fails EVERY assertion idiom
    the suite uses (IDIOMS, listed once);
  * the same values in the halo ring or in a slot that is not prognostic (node slot 3, interface slots 0, 1, 2, 4) change nothing;
  * on finite data the helpers return the floats they returned before: `==` against verbatim copies of the former helpers (_old_*) on
    200 seeded cases, magnitudes 1e-300 .. 1e300, all-zero references, single differing entries and negative zeros among them;
  * another number of patches or another shape raises instead of shortening (zip) or broadcasting (a - b) the comparison;
  * the former helper, kept verbatim, still returns zeros on the NaN case: what was fixed, on record."""
import itertools
import numpy as np
import pytest
import golden_util as gu
import levels_common as lc

INF = float("inf")
VALUES = [float("nan"), INF, -INF]
VALUE_IDS = ["nan", "+inf", "-inf"]
NP, NA, NB, L, NT = 3, 6, 6, 3, 2
SIDES = ["got", "ref", "both"]

# Every way the suite turns an error list into a verdict (True: the comparison PASSES).  The lossy ones among them (`not (x > tol)`,
# `if x > tol: bad.append`) are listed on purpose: an inf fails them too, which is why inf and not NaN is what the helpers return.
IDIOMS = [
    ("max(errs) <= tol", lambda errs: max(errs) <= 1e-10),
    ("max(errs) <= EXACT", lambda errs: max(errs) <= 0.0),
    ("max(errs) == 0.0", lambda errs: max(errs) == 0.0),
    ("max(errs) < 1e-12", lambda errs: max(errs) < 1e-12),
    ("not max(errs) <= EXACT -> bad", lambda errs: not (not max(errs) <= 0.0)),
    ("not (max(errs) > tol)", lambda errs: not (max(errs) > 1e-10)),
    ("if e > tol: bad.append", lambda errs: not [e for e in errs if e > 1e-10]),
    ("all(e <= tol)", lambda errs: all(e <= 1e-10 for e in errs)),
    ("max(reversed) <= tol", lambda errs: max(list(errs)[::-1]) <= 1e-10),
    ("np.max(errs) <= tol", lambda errs: bool(np.max(errs) <= 1e-10)),
    ("differs: tol < max(errs) < inf", lambda errs: 1e-6 < max(errs) < INF),
]


def _fails_every_idiom(errs):
    return [name for name, passes in IDIOMS if passes(errs)]      # the idioms that would have let it through: must be empty


def _state(seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-1.0, 1.0, (5, NA, NB, L)), rng.uniform(-1.0, 1.0, (5, NA, NB, L + 1))) for _ in range(NP)]


def _tracers(seed=0):
    rng = np.random.default_rng(100 + seed)
    return [rng.uniform(0.0, 1.0, (NT, NA, NB, L)) for _ in range(NP)]


def _copy(states):
    return [(n.copy(), e.copy()) for n, e in states]


def _plant(states, p, c, value, where=(2, 3, 1)):
    """value into prognostic variable c of patch p (W lives on the interfaces)."""
    states[p][1 if c == 3 else 0][(c,) + where] = value


def _planted_pairs(c, p, side, value, where=(2, 3, 1)):
    got, ref = _state(), _state()
    if side in ("got", "both"):
        _plant(got, p, c, value, where)
    if side in ("ref", "both"):
        _plant(ref, p, c, value, where)
    return got, ref


PLANTS = list(itertools.product(range(3), range(NP), SIDES))      # (value, patch, side)
PLANT_IDS = ["%s-p%d-%s" % (VALUE_IDS[v], p, s) for v, p, s in PLANTS]


# ---- verbatim copies of the former helpers (golden_util.py before this file existed); do not repair them ----

def _old_tracer_errors(got, ref):
    """Max abs difference per tracer over interior nodes, relative to the max abs value of that tracer in ``ref``."""
    nt = ref[0].shape[0]
    errs = []
    for c in range(nt):
        num = max(float(np.max(np.abs(a[c, 1:-1, 1:-1] - b[c, 1:-1, 1:-1]))) for a, b in zip(got, ref))
        den = max(float(np.max(np.abs(b[c, 1:-1, 1:-1]))) for b in ref)
        errs.append(num / den if den > 0 else num)
    return errs


def _old_prognostic_errors(got, ref, interior=True):
    """Max abs difference per variable (U,V,rhotheta,W,rho) over the prognostic slots, relative to the
    max abs value of that variable in ``ref``."""
    errs = []
    for c in range(5):
        m = 0.0; s = 0.0
        loc = 1 if c == 3 else 0
        for (gn, ge), (rn, re_) in zip(got, ref):
            a = (ge if loc else gn)[c]; b = (re_ if loc else rn)[c]
            if interior:
                a = a[1:-1, 1:-1]; b = b[1:-1, 1:-1]
            m = max(m, float(np.max(np.abs(a - b)))); s = max(s, float(np.max(np.abs(b))))
        errs.append(m / s if s > 0 else m)
    return errs


def _old_interp_rel(x, y):
    return max(float(np.max(np.abs(x[c] - y[c])) / max(np.max(np.abs(y[c])), 1e-300)) for c in range(x.shape[0]))


# ---- planted values that must fail ----

@pytest.mark.parametrize("interior", [True, False])
@pytest.mark.parametrize("c", range(5), ids=["U", "V", "rhotheta", "W", "rho"])
def test_prognostic_errors_planted_values_fail_every_idiom(c, interior):
    for (v, p, side), tag in zip(PLANTS, PLANT_IDS):
        spots = [(2, 3, 1), (1, 1, 0), (NA - 2, NB - 2, L - 1 + (c == 3))]      # interior nodes: the middle, the two corners
        if not interior:
            spots += [(0, 2, 1), (NA - 1, NB - 1, 0)]      # without `interior` the halo ring is compared as well
        for where in spots:
            got, ref = _planted_pairs(c, p, side, VALUES[v], where)
            errs = gu.prognostic_errors(got, ref, interior=interior)
            assert isinstance(errs, list) and len(errs) == 5 and all(type(e) is float for e in errs), (tag, errs)
            assert errs[c] == INF and all(errs[k] == 0.0 for k in range(5) if k != c), (tag, where, errs)
            assert _fails_every_idiom(errs) == [], (tag, where, errs)
            assert _fails_every_idiom(errs[:3] if c < 3 else errs[3:]) == [], (tag, where)      # (the shallow-water tests slice [:3])


@pytest.mark.parametrize("c", range(NT))
def test_tracer_errors_planted_values_fail_every_idiom(c):
    for (v, p, side), tag in zip(PLANTS, PLANT_IDS):
        for where in ((2, 3, 1), (1, 1, 0), (NA - 2, NB - 2, L - 1)):
            got, ref = _tracers(), _tracers()
            for arr, on in ((got, side in ("got", "both")), (ref, side in ("ref", "both"))):
                if on:
                    arr[p][(c,) + where] = VALUES[v]
            errs = gu.tracer_errors(got, ref)
            assert isinstance(errs, list) and len(errs) == NT and all(type(e) is float for e in errs), (tag, errs)
            assert errs[c] == INF and errs[1 - c] == 0.0, (tag, where, errs)
            assert _fails_every_idiom(errs) == [], (tag, where, errs)


def test_interp_rel_and_field_distance_planted_values_fail_every_idiom():
    rng = np.random.default_rng(5)
    base = rng.uniform(-1.0, 1.0, (5, 4, 7))
    for v, side, c, where in itertools.product(range(3), SIDES, range(5), [(0, 0), (3, 6), (2, 1)]):
        x, y = base.copy(), base.copy()
        if side in ("got", "both"):
            x[(c,) + where] = VALUES[v]
        if side in ("ref", "both"):
            y[(c,) + where] = VALUES[v]
        r = gu.interp_rel(x, y)
        assert r == INF and _fails_every_idiom([r]) == [], (VALUE_IDS[v], side, c, where, r)
        dist = lc.field_distance(x, y, base)
        assert dist[c] == INF and all(dist[k] == 0.0 for k in range(5) if k != c) and _fails_every_idiom(dist) == [], (VALUE_IDS[v], side, c, dist)
    full = base.copy(); full[1, 2, 2] = float("nan")      # the scale of field_distance counts as well
    assert lc.field_distance(base, base, full)[1] == INF
    assert gu.interp_rel(base, base) == 0.0 and lc.field_distance(base, base, base) == [0.0] * 5


class _Fake:
    """An engine (sync / download_state) or an oracle (get_state) that hands out prepared states."""
    def __init__(self, states, tracers=None, prect=None):
        self.states, self.tracers, self.prect, self.synced = states, tracers, prect, 0

    def sync(self):
        self.synced += 1

    def download_state(self, i):
        return self.states[i]

    get_state = download_state

    def download_tracers(self, i):
        return self.tracers[i]

    def download_precipitation(self, reset=False):
        return self.prect


@pytest.mark.parametrize("c", range(5), ids=["U", "V", "rhotheta", "W", "rho"])
def test_cmp_of_parity_common_fails_on_planted_values(c):
    from parity_common import _cmp
    clean = _state()
    e, o = _Fake({2: clean}), _Fake({1: _copy(clean)})
    assert _cmp(e, o, 2, 1, 0.0, "clean") == [0.0] * 5 and e.synced == 1
    for (v, p, side), tag in zip(PLANTS, PLANT_IDS):
        got, ref = _planted_pairs(c, p, side, VALUES[v])
        for tol in (0.0, 1e-10, 1e300):
            with pytest.raises(AssertionError):
                _cmp(_Fake({0: got}), _Fake({0: ref}), 0, 0, tol, tag)


@pytest.mark.parametrize("c", range(5), ids=["U", "V", "rhotheta", "W", "rho"])
def test_stage_walk_wrappers_fail_on_planted_values(c):
    """_errs / _terrs / _finite of test_gpu_stage_walk_segments.py (imported by test_gpu_tracer_column_shapes.py as well)."""
    from test_gpu_stage_walk_segments import _errs, _terrs, _finite
    assert _errs(_state(), _state()) == [0.0] * 5 and _terrs(_tracers(), _tracers()) == [0.0] * NT and _finite(_state())
    for (v, p, side), tag in zip(PLANTS, PLANT_IDS):
        got, ref = _planted_pairs(c, p, side, VALUES[v])
        errs = _errs(got, ref)
        assert errs[c] == INF and _fails_every_idiom(errs) == [], (tag, errs)
        assert not (_finite(got) and _finite(ref)), tag
        if c < NT:
            tg, tr = _tracers(), _tracers()
            for arr, on in ((tg, side in ("got", "both")), (tr, side in ("ref", "both"))):
                if on:
                    arr[p][c, 2, 3, 1] = VALUES[v]
            terrs = _terrs(tg, tr)
            assert terrs[c] == INF and _fails_every_idiom(terrs) == [], (tag, terrs)


def _dcmip_toy(ntr=4):
    """A fixture dict, a grid and the matching device-side arrays for test_gpu_dcmip_physics._check_call: after the call every entry is
    the starting value + 1 (stored, as in the real fixture, as the XOR with the start), W and the tracers beyond the third stay."""
    rng = np.random.default_rng(9)
    d, states, tracers, prect = {}, [], [], {}
    for p in range(NP):
        node, redge, tr = rng.uniform(1.0, 2.0, (4, 4, 4, L)), rng.uniform(1.0, 2.0, (4, 4, L + 1)), rng.uniform(1.0, 2.0, (ntr, 4, 4, L))
        pr = rng.uniform(0.0, 1.0, (NA, NB))
        d["state/s/p%d/node" % p], d["state/s/p%d/redge" % p], d["state/s/p%d/tracers" % p], d["prect/c/p%d" % p] = node, redge, tr, pr
        d["xor/c/p%d/node" % p] = np.bitwise_xor(node.view(np.uint64), (node + 1.0).view(np.uint64))
        d["xor/c/p%d/tracers" % p] = np.bitwise_xor(np.ascontiguousarray(tr[:3]).view(np.uint64), (tr[:3] + 1.0).view(np.uint64))
        n, e, t = np.zeros((5, NA, NB, L)), np.zeros((5, NA, NB, L + 1)), np.zeros((ntr, NA, NB, L))
        n[[0, 1, 2, 4], 1:-1, 1:-1] = node + 1.0; e[3, 1:-1, 1:-1] = redge
        t[:3, 1:-1, 1:-1] = tr[:3] + 1.0; t[3:, 1:-1, 1:-1] = tr[3:]
        states.append((n, e)); tracers.append(t); prect[p] = pr.copy()

    class _P:
        def __init__(self, index):
            self.index = index

    class _G:
        patches = [_P(p) for p in range(NP)]
    return d, _G(), states, tracers, prect


def test_dcmip_check_call_fails_on_planted_values():
    from test_gpu_dcmip_physics import _check_call
    d, g, states, tracers, prect = _dcmip_toy()
    assert _check_call(_Fake({0: states}, {0: tracers}, prect), d, g, "s", "c") == 0.0
    scalar = [(name, f) for name, f in IDIOMS]
    for v, p in itertools.product(range(3), range(NP)):
        # the device's side: each prognostic variable, a tracer the physics writes, one it leaves alone, the precipitation
        for what in ("U", "V", "rhotheta", "W", "rho", "tracer1", "tracer3", "prect"):
            d, g, states, tracers, prect = _dcmip_toy()
            if what in ("U", "V", "rhotheta", "W", "rho"):
                _plant(states, p, ["U", "V", "rhotheta", "W", "rho"].index(what), VALUES[v])
            elif what == "prect":
                prect[p][2, 2] = VALUES[v]
            else:
                tracers[p][int(what[-1]), 2, 3, 1] = VALUES[v]
            worst = _check_call(_Fake({0: states}, {0: tracers}, prect), d, g, "s", "c")
            assert worst == INF and [n for n, f in scalar if f([worst])] == [], (VALUE_IDS[v], p, what, worst)
        # the fixture's side, and the same value on both
        for both in (False, True):
            d, g, states, tracers, prect = _dcmip_toy()
            d["state/s/p%d/redge" % p][1, 2, 1] = VALUES[v]
            if both:
                states[p][1][3, 2, 3, 1] = VALUES[v]
            worst = _check_call(_Fake({0: states}, {0: tracers}, prect), d, g, "s", "c")
            assert worst == INF and [n for n, f in scalar if f([worst])] == [], (VALUE_IDS[v], p, both, worst)
    d, g, states, tracers, prect = _dcmip_toy()      # a halo value or a slot that is not prognostic is not compared
    states[0][0][3] = float("nan"); states[1][1][[0, 1, 2, 4]] = INF; states[2][0][0, 0, :, :] = -INF; tracers[1][:, :, NB - 1] = float("nan")
    assert _check_call(_Fake({0: states}, {0: tracers}, prect), d, g, "s", "c") == 0.0
    d, g, states, tracers, prect = _dcmip_toy()      # one level where the fixture has L: np would broadcast it
    d["state/s/p1/redge"] = d["state/s/p1/redge"][..., :1]
    with pytest.raises(ValueError):
        _check_call(_Fake({0: states}, {0: tracers}, prect), d, g, "s", "c")


def test_worse_keeps_what_max_drops():
    assert gu.worse(0.0, 3.0) == 3.0 and gu.worse(3.0, 0.0) == 3.0 and gu.worse(0.0, 0.0) == 0.0
    for v in VALUES:
        assert gu.worse(0.0, v) == INF and gu.worse(v, 0.0) == INF and gu.worse(v, v) == INF
    assert max(0.0, float("nan")) == 0.0      # what the folds were written with


# ---- planted values that must not fail ----

@pytest.mark.parametrize("v", range(3), ids=VALUE_IDS)
def test_values_outside_the_compared_region_change_nothing(v):
    for p, side in itertools.product(range(NP), SIDES):
        got, ref = _state(), _state()
        tg, tr = _tracers(), _tracers()
        for (states, trs), on in (((got, tg), side in ("got", "both")), ((ref, tr), side in ("ref", "both"))):
            if not on:
                continue
            node, redge = states[p]
            node[3] = VALUES[v]                      # node slot 3 (W on nodes: derived)
            redge[[0, 1, 2, 4]] = VALUES[v]          # interface slots 0, 1, 2, 4 (derived or scratch)
            for arr in (node, redge, trs[p]):        # the halo ring of every slot
                arr[:, 0] = VALUES[v]; arr[:, -1] = VALUES[v]; arr[:, :, 0] = VALUES[v]; arr[:, :, -1] = VALUES[v]
        assert gu.prognostic_errors(got, ref) == [0.0] * 5, (p, side)
        assert gu.tracer_errors(tg, tr) == [0.0] * NT, (p, side)
    got, ref = _state(), _state()                    # without `interior` the ring counts, the other slots still do not
    got[1][0][3] = VALUES[v]; ref[2][1][[0, 1, 2, 4]] = VALUES[v]
    assert gu.prognostic_errors(got, ref, interior=False) == [0.0] * 5


# ---- unchanged on finite data ----

def _finite_case(k):
    """Case k of 200: got and ref states and tracers, finite.  The kinds rotate: ordinary magnitudes with rounding-size differences; tiny
    (1e-300) and huge (1e300) ones; a reference that is zero in some or all variables; one differing entry; negative zeros; equal."""
    rng = np.random.default_rng(1000 + k)
    kind = k % 8
    mag = [1.0, 1e-300, 1e300, 1e-150, 1e150, 1.0, 1.0, 1.0][kind] if kind < 5 else float(10.0 ** rng.uniform(-300.0, 300.0))
    ref = [(mag * rng.uniform(-1.0, 1.0, (5, NA, NB, L)), mag * rng.uniform(-1.0, 1.0, (5, NA, NB, L + 1))) for _ in range(NP)]
    tref = [mag * rng.uniform(-1.0, 1.0, (NT, NA, NB, L)) for _ in range(NP)]
    if kind == 5:        # all-zero reference, wholly (every other time) or in two variables and one tracer
        for (n, e), t in zip(ref, tref):
            if (k // 8) % 2:
                n[:] = 0.0; e[:] = 0.0; t[:] = 0.0
            else:
                n[[1, 4]] = 0.0; e[3] = 0.0; t[0] = 0.0
    if kind == 6:        # negative zeros on the reference's side, positive on the other
        for (n, e), t in zip(ref, tref):
            n[0] = -0.0; n[2, 2:4] = -0.0; e[3, :, :, 0] = -0.0; t[1] = -0.0
    got, tgot = _copy(ref), [t.copy() for t in tref]
    if kind == 6:
        for (n, e), t in zip(got, tgot):
            n[0] = 0.0; e[3, :, :, 0] = 0.0; t[1] = 0.0
    elif kind == 7:      # a single differing entry, in one patch
        p = k % NP
        got[p][0][k % 5 if k % 5 != 3 else 0, 2, 2, 1] *= 1.0 + 2.0 ** -40
        got[p][1][3, 3, 1, 2] += mag * 2.0 ** -30
        tgot[p][k % NT, 1, 4, 0] -= mag * 2.0 ** -35
    elif k % 3:          # rounding-size to large differences everywhere (k % 3 == 0: equal)
        eps = float(10.0 ** rng.uniform(-16.0, 0.0))
        got = [(n * (1.0 + eps * rng.uniform(-1.0, 1.0, n.shape)), e * (1.0 + eps * rng.uniform(-1.0, 1.0, e.shape)) + (mag * eps if kind == 5 else 0.0))
               for n, e in got]
        tgot = [t * (1.0 + eps * rng.uniform(-1.0, 1.0, t.shape)) + (mag * eps if kind == 5 else 0.0) for t in tgot]
    return got, ref, tgot, tref


def test_finite_data_gives_the_former_floats():
    seen = set()
    with np.errstate(all="ignore"):
        for k in range(200):
            got, ref, tgot, tref = _finite_case(k)
            assert all(np.isfinite(n).all() and np.isfinite(e).all() for n, e in got + ref) and all(np.isfinite(t).all() for t in tgot + tref), k
            for interior in (True, False):
                new, old = gu.prognostic_errors(got, ref, interior=interior), _old_prognostic_errors(got, ref, interior=interior)
                assert new == old and all(type(v) is float for v in new), (k, interior, new, old)
                seen.update(old)
            new, old = gu.tracer_errors(tgot, tref), _old_tracer_errors(tgot, tref)
            assert new == old and all(type(v) is float for v in new), (k, new, old)
            x, y = np.stack([n[:, 2] for n, _ in got]).reshape(NP * 5, -1), np.stack([n[:, 2] for n, _ in ref]).reshape(NP * 5, -1)
            assert gu.interp_rel(x, y) == float(_old_interp_rel(x, y)), k
            seen.update(old)
    assert 0.0 in seen and len(seen) > 300 and min(v for v in seen if v > 0.0) < 1e-15 and max(seen) > 1e-3, len(seen)      # the cases are not all alike


# ---- length and shape ----

def test_another_patch_count_or_shape_raises():
    got, ref, tg, tr = _state(), _state(), _tracers(), _tracers()
    for a, b in ((got[:2], ref), (got, ref[:1]), ([], ref), (got, [])):
        with pytest.raises(ValueError):
            gu.prognostic_errors(a, b)
    for a, b in ((tg[:2], tr), (tg, tr[1:])):
        with pytest.raises(ValueError):
            gu.tracer_errors(a, b)
    assert gu.prognostic_errors(got[:2], ref[:2]) == [0.0] * 5      # a subset: both sides sliced, where the reader sees it
    one_level = [(n[..., :1].copy(), e[..., :1].copy()) for n, e in got]      # a level axis of 1 broadcasts against L
    assert _old_prognostic_errors(one_level, ref)[0] > 0.0
    for interior in (True, False):
        with pytest.raises(ValueError):
            gu.prognostic_errors(one_level, ref, interior=interior)
        with pytest.raises(ValueError):
            gu.prognostic_errors(got, [(n[:, :-1], e[:, :-1]) for n, e in ref], interior=interior)
    with pytest.raises(ValueError):
        gu.tracer_errors([t[..., :1] for t in tg], tr)
    with pytest.raises(ValueError):
        gu.tracer_errors([t[:1] for t in tg], tr)      # fewer tracers on one side
    x = np.ones((5, 4, 7))
    for y in (x[:4], x[:, :1], x[:, :, :1]):
        with pytest.raises(ValueError):
            gu.interp_rel(x, y)
        with pytest.raises(ValueError):
            gu.interp_rel(y, x)
    with pytest.raises(ValueError):
        lc.field_distance(x, x[:, :1], x)


# ---- regression control ----

def test_the_former_helpers_pass_a_nan():
    """What was fixed: the verbatim copies return zeros for a NaN in rho*theta of an interior node, in patch 0 or patch 1, and
    [0.0, nan] for a NaN in the first patch's tracer 1, which `max(errs) == 0.0` lets through.  If someone repairs the copies this fails:
    they are the record of the former behaviour and the yardstick of test_finite_data_gives_the_former_floats."""
    for p in (0, 1):
        got, ref = _planted_pairs(2, p, "got", float("nan"))
        assert _old_prognostic_errors(got, ref) == [0.0] * 5
        assert gu.prognostic_errors(got, ref) == [0.0, 0.0, INF, 0.0, 0.0]
    tg, tr = _tracers(), _tracers()
    tg[1][0, 2, 2, 1] = float("nan")      # any patch but the first: dropped
    assert _old_tracer_errors(tg, tr) == [0.0, 0.0] and gu.tracer_errors(tg, tr) == [INF, 0.0]
    tg, tr = _tracers(), _tracers()
    tg[0][1, 2, 2, 1] = float("nan")      # the first patch: [0.0, nan], and max([0.0, nan]) == 0.0
    old = _old_tracer_errors(tg, tr)
    assert old[0] == 0.0 and old[1] != old[1] and max(old) == 0.0
    assert gu.tracer_errors(tg, tr) == [0.0, INF]
