"""Shared pieces of the DCMIP2016 column-physics tests: the fixture decoding and a plain-Python restatement of the reference's
covector transforms (src/atm/CubedSphereTrans.cpp:549-729) evaluated with the host's libm (math), term by term."""
import math
import numpy as np
import golden_util as gu

COMBOS = [(pb, pr) for pb in (0, 1) for pr in (0, 1)]
GRID = "ne2_L6_p6"


def load_case(case):
    """The per-call fixture of case "tc" (tropical cyclone) or "bw" (moist baroclinic wave): its two files joined (the calls
    on the moistened starting state are kept in a file of their own, tests/golden/make_golden_dcmip.py)."""
    d = gu.load("dcmip_%s_%s.npz" % (case, GRID))
    d.update(gu.load("dcmip_%s_moist_%s.npz" % (case, GRID)))
    return d


def decode_after(d, start, call, p, what):
    """State of patch p after a call (fixture key xor/<call>/p<p>/<what>): stored as the bitwise XOR with the starting state."""
    base = d["state/%s/p%d/%s" % (start, p, what)]
    x = d["xor/%s/p%d/%s" % (call, p, what)]
    if what == "tracers":
        base = base[:3]
    return np.bitwise_xor(np.ascontiguousarray(base).view(np.uint64), x).view(np.float64)


def heights(d, P):
    """Level and interface heights of patch P as [na][nb][L] / [na][nb][L+1] (the fixture keeps one column: no topography)."""
    zl, zi = d["p%d/dcmip_z_levels" % P.index], d["p%d/dcmip_z_interfaces" % P.index]
    return (np.ascontiguousarray(np.broadcast_to(zl, (P.na, P.nb, zl.size))),
            np.ascontiguousarray(np.broadcast_to(zi, (P.na, P.nb, zi.size))))


def rll_from_abp(X, Y, p, ua, ub):
    """CubedSphereTrans::CoVecTransRLLFromABP, as written there."""
    d2 = 1.0 + X * X + Y * Y
    if p > 3 and abs(X) < 1.0e-13 and abs(Y) < 1.0e-13:
        return (ua if p == 4 else -ua), ub
    if p <= 3:
        ulon = d2 / (1.0 + X * X) * ua + d2 * X * Y / (1.0 + X * X) / (1.0 + Y * Y) * ub
        ulat = d2 / math.sqrt(1.0 + X * X) / (1.0 + Y * Y) * ub
        lat = math.atan(Y / math.sqrt(1.0 + X * X))
        return ulon * math.cos(lat), ulat
    r2 = X * X + Y * Y
    r = math.sqrt(r2)
    if p == 4:
        ulon = -d2 * Y / (1.0 + X * X) / r2 * ua + d2 * X / (1.0 + Y * Y) / r2 * ub
        ulat = -d2 * X / (1.0 + X * X) / r * ua - d2 * Y / (1.0 + Y * Y) / r * ub
    else:
        ulon = +d2 * Y / (1.0 + X * X) / r2 * ua - d2 * X / (1.0 + Y * Y) / r2 * ub
        ulat = +d2 * X / (1.0 + X * X) / r * ua + d2 * Y / (1.0 + Y * Y) / r * ub
    lat = 0.5 * math.pi - math.atan(math.sqrt(X * X + Y * Y))
    return ulon * math.cos(lat), ulat


def abp_from_rll(X, Y, p, ulon, ulat):
    """CubedSphereTrans::CoVecTransABPFromRLL, as written there."""
    d2 = 1.0 + X * X + Y * Y
    if p > 3 and abs(X) < 1.0e-13 and abs(Y) < 1.0e-13:
        return (ulon if p == 4 else -ulon), ulat
    if p <= 3:
        lat = math.atan(Y / math.sqrt(1.0 + X * X))
        ulon = ulon / math.cos(lat)
        ua = (1.0 + X * X) / d2 * ulon - X * Y * math.sqrt(1.0 + X * X) / d2 * ulat
        ub = math.sqrt(1.0 + X * X) * (1.0 + Y * Y) / d2 * ulat
        return ua, ub
    r = math.sqrt(X * X + Y * Y)
    if p == 4:
        lat = 0.5 * math.pi - math.atan(math.sqrt(X * X + Y * Y))
        ulon = ulon / math.cos(lat)
        ua = -Y * (1.0 + X * X) / d2 * ulon - X * (1.0 + X * X) / (d2 * r) * ulat
        ub = +X * (1.0 + Y * Y) / d2 * ulon - Y * (1.0 + Y * Y) / (d2 * r) * ulat
    else:
        lat = -0.5 * math.pi + math.atan(math.sqrt(X * X + Y * Y))
        ulon = ulon / math.cos(lat)
        ua = +Y * (1.0 + X * X) / d2 * ulon + X * (1.0 + X * X) / (d2 * r) * ulat
        ub = -X * (1.0 + Y * Y) / d2 * ulon + Y * (1.0 + Y * Y) / (d2 * r) * ulat
    return ua, ub


# ---- the slim fixtures at further shapes (written by tests/golden/make_golden_dcmip.py from this table; what each reaches: DESIGN.md section 2) ----
# id -> (ne, L, ztop, dt, cases).  Each file holds cfg/, phys/, per patch lat, a_nodes, b_nodes and one column of level and interface
# heights, the MOIST starting state, its five calls as XOR against it, PRECT of each call and the branch counters -- no metric, no
# operators: the physics reads none of them.  The engine's grid object does want a metric, so it is golden_util.make_grid's own (the
# same cubed sphere, synthesised) and everything the physics reads is uploaded from the file (slim_engine).
SLIM = {
    "A": (3, 17, 4500, 300, ("tc",)),
    "B": (1, 53, 12000, 600, ("tc", "bw")),
    "Bp": (1, 53, 4500, 600, ("tc",)),
    "C": (1, 54, 12000, 600, ("tc",)),
    "D": (1, 30, 30000, 300, ("tc", "bw")),
    "E": (1, 4, 4500, 300, ("tc",)),      # (the reference's column solve refuses L = 3: 4 is the smallest count it runs)
}
SLIM_FILES = [(sid, case) for sid, s in SLIM.items() for case in s[4]]
SLIM_IDS = ["%s_%s" % f for f in SLIM_FILES]
INFO_LOCAL_COLUMNS, INFO_PHYSICS_KERNEL = 0, 24      # tmx_info (include/tempest_mi355x.h)
# bytes of dynamic LDS k_dcmip<pbl, prec, true> is launched with, 6 x L x 64 doubles where they fit 160 KB (C: they do not)
LDS_BYTES = {"A": 52224, "B": 162816, "Bp": 162816, "C": 0, "D": 92160, "E": 12288}
_slim, _grids = {}, {}


def slim_name(sid, case):
    ne, L, ztop, dt, _ = SLIM[sid]
    return "dcmip_%s_slim_ne%d_L%d_z%d_dt%d_p6" % (case, ne, L, ztop, dt)


def load_slim(sid, case="tc"):
    """The slim fixture of shape sid and case, its parts joined (a file above 1 MiB is cut by calls: <name>.part1.npz, ...).
    Loaded once and shared: nobody writes to it."""
    if (sid, case) not in _slim:
        import glob
        import os
        stem = slim_name(sid, case)
        d = gu.load(stem + ".npz")
        for part in sorted(glob.glob(os.path.join(gu.GOLDEN, stem + ".part*.npz"))):
            d.update(gu.load(os.path.basename(part)))
        for v in d.values():
            v.setflags(write=False)
        _slim[(sid, case)] = d
    return _slim[(sid, case)]


def slim_test(d):
    return int(d["cfg/test"][0])


def slim_calls(d):
    """(test, pbl, prec) of the recorded calls, in the generator's order."""
    t = slim_test(d)
    return [(t, pb, pr) for pb, pr in COMBOS] + [(3, 0, 0)]


def call_key(t, pb, pr):
    return "moist_t%d_pbl%d_prec%d" % (t, pb, pr)


def slim_grid(d):
    """make_grid's grid at the fixture's ne, L and ztop with its tracer count (shared between the tests of one shape)."""
    key = (int(d["cfg/ne"][0]), int(d["cfg/levels"][0]), float(d["cfg/ztop"][0]), int(d["cfg/ntracers"][0]))
    if key not in _grids:
        _grids[key] = gu.make_grid(key[0], key[1], 6, key[2], ntracers=key[3])[0]
    return _grids[key]


def slim_engine(d, g, zl=None, zi=None, **kw):
    """An engine on g with the physics' inputs from fixture d (zl, zi: per-patch height arrays instead of the fixture's columns)."""
    from tempestmodel_amd.engine import Engine
    e = Engine(g, **kw)
    try:
        h = [heights(d, P) for P in g.patches]
        e.set_level_heights([x[0] for x in h] if zl is None else zl)
        e.set_dcmip_inputs(latitude=[d["p%d/lat" % P.index] for P in g.patches], a_nodes=[d["p%d/a_nodes" % P.index] for P in g.patches],
                           b_nodes=[d["p%d/b_nodes" % P.index] for P in g.patches], z_interfaces=[x[1] for x in h] if zi is None else zi,
                           earth_radius=float(d["phys/earth_radius"][0]))
    except Exception:
        e.close()
        raise
    return e


def physics_kernel_code(pbl, prec, lds_bytes):
    """TMX_INFO_PHYSICS_KERNEL of a k_dcmip launch: family 3 | pbl << 2 | prec << 3 | bytes of dynamic LDS << 4."""
    return 3 | pbl << 2 | prec << 3 | lds_bytes << 4


def kessler_kernel_code(kt):
    """... of a Kessler launch: k_kessler_tile with kt wavefronts per column tile (family 2), kt = 0: k_kessler (family 1)."""
    return (2 | kt << 4) if kt else 1


def mismatches(e, d, g, want_node, want_tr, want_pr, patches=None):
    """What of the device state differs from the expected one, as a list of strings (empty: all equal).  want_node[p] is
    [4][..][..][L] (U, V, rho*theta, rho on the interior), want_tr[p] the first three tracers, want_pr[p] PRECT on the interior; W and
    the tracers beyond the third are compared with fixture d's starting state.  np.array_equal throughout: a NaN is a miss."""
    got, gt, pr = e.download_state(0), e.download_tracers(0), e.download_precipitation()
    bad = []
    for p in (e.local_patches if patches is None else patches):
        n, w = got[p]
        t = gt[p][:, 1:-1, 1:-1]
        for what, a, b in (("U,V,rho*theta,rho", n[[0, 1, 2, 4], 1:-1, 1:-1], want_node[p]), ("W", w[3, 1:-1, 1:-1], d["state/moist/p%d/redge" % p]),
                           ("tracers 0-2", t[:3], want_tr[p]), ("tracers 3+", t[3:], d["state/moist/p%d/tracers" % p][3:]),
                           ("PRECT", pr[p][1:-1, 1:-1], want_pr[p])):
            if not np.array_equal(a, b):
                with np.errstate(invalid="ignore"):
                    rel = float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300) if a.shape == np.shape(b) and np.size(b) else float("nan")
                bad.append("patch %d %s: %d of %d entries differ, %d not finite, max relative %.3e"
                           % (p, what, int(np.sum(a != b)), a.size, int(np.sum(~np.isfinite(a))), rel))
    return bad


def recorded(d, call, npatch=6):
    """(node, tracers, PRECT interior) per patch of a recorded call of fixture d."""
    return ([decode_after(d, "moist", call, p, "node") for p in range(npatch)], [decode_after(d, "moist", call, p, "tracers") for p in range(npatch)],
            [d["prect/%s/p%d" % (call, p)][1:-1, 1:-1] for p in range(npatch)])
