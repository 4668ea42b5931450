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
