"""DCMIP2016 column physics (tmx_physics_dcmip2016), the parts that run without a GPU: the per-node covector coefficients the host
forms at set-up against a plain restatement of the reference's transforms, and what the reference fixtures must show to be
worth pinning."""
import ctypes as C
import math
import numpy as np
import pytest
import golden_util as gu
import dcmip_common as dc

PD = C.POINTER(C.c_double)


def _lib():
    from tempestmodel_amd.engine import load_library
    return load_library()


def _coefficients(lib, panel, a, b):
    out = np.zeros(11)
    assert lib.tmx_debug_dcmip_node_coefficients(panel, a, b, out.ctypes.data_as(PD)) == 0
    return out


def _apply_rll(c, ua, ub):
    return (c[0] * ua + c[1] * ub) * c[4], c[2] * ua + c[3] * ub


def _apply_abp(c, ulon, ulat):
    lon = ulon / c[5]
    return c[6] * lon + c[7] * ulat, c[8] * lon + c[9] * ulat


def test_covector_coefficients_match_the_reference_transforms():
    """Both directions on all six panels, at GLL-like and random angles, the polar panel centres (|X|, |Y| < 1e-13) included:
    coefficient x component products give the reference's doubles bit for bit (0.0 == -0.0 where a term is absent)."""
    lib = _lib()
    rng = np.random.default_rng(7)
    angles = list(rng.uniform(-math.pi / 4, math.pi / 4, size=(40, 2)))
    angles += [(0.0, 0.0), (1e-14, -3e-14), (0.0, 0.3), (-0.2, 0.0), (math.pi / 4, -math.pi / 4)]
    n = 0
    for panel in range(6):
        for a, b in angles:
            c = _coefficients(lib, panel, float(a), float(b))
            X, Y = math.tan(a), math.tan(b)
            for ua, ub in rng.normal(scale=30.0, size=(4, 2)):
                got = _apply_rll(c, float(ua), float(ub))
                ref = dc.rll_from_abp(X, Y, panel, float(ua), float(ub))
                assert got[0] == ref[0] and got[1] == ref[1], (panel, a, b, got, ref)
                got2 = _apply_abp(c, ref[0], ref[1])
                ref2 = dc.abp_from_rll(X, Y, panel, ref[0], ref[1])
                assert got2[0] == ref2[0] and got2[1] == ref2[1], (panel, a, b, got2, ref2)
                # round trip: back to the components within rounding
                assert abs(got2[0] - ua) <= 1e-12 * (abs(ua) + abs(ub)) and abs(got2[1] - ub) <= 1e-12 * (abs(ua) + abs(ub))
                n += 1
    assert n == 6 * len(angles) * 4
    # the panel-centre branch of the polar panels is the identity up to the sign of u_lon
    c4, c5 = _coefficients(lib, 4, 0.0, 0.0), _coefficients(lib, 5, 0.0, 0.0)
    assert list(c4[:10]) == [1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0]
    assert list(c5[:10]) == [-1.0, 0.0, 0.0, 1.0, 1.0, 1.0, -1.0, 0.0, 0.0, 1.0]
    assert lib.tmx_debug_dcmip_node_coefficients(6, 0.0, 0.0, np.zeros(11).ctypes.data_as(PD)) != 0


def test_test1_surface_temperature_is_the_moist_baroclinic_wave_profile():
    """Tsurf of test 1 (dcmip_physics_z_v1.f90:204-212) as the host forms it, against the source expression evaluated in
    Python (the folded constants of the compiled Fortran may move the last bit, nothing more)."""
    lib = _lib()
    lib.tmx_debug_dcmip_tsurf.argtypes = [C.c_double, PD]
    pi = 4.0 * math.atan(1.0)
    T00, u0, rair, a, omega, q0 = 288.0, 35.0, 287.0, 6371220.0, 7.29212e-5, 0.021
    latw, eta0 = 2.0 * pi / 9.0, 0.252
    etav = (1.0 - eta0) * 0.5 * pi
    zvir = (461.5 / 287.0) - 1.0
    for lat in np.linspace(-1.5, 1.5, 61):
        s, c = math.sin(lat), math.cos(lat)
        ref = (T00 + pi * u0 / rair * 1.5 * math.sin(etav) * math.cos(etav) ** 0.5 *
               ((-2.0 * s ** 6 * (c ** 2 + 1.0 / 3.0) + 10.0 / 63.0) * u0 * math.cos(etav) ** 1.5 +
                (8.0 / 5.0 * c ** 3 * (s ** 2 + 2.0 / 3.0) - pi / 4.0) * a * omega * 0.5)) / (1.0 + zvir * q0 * math.exp(-(lat / latw) ** 4))
        out = C.c_double()
        assert lib.tmx_debug_dcmip_tsurf(float(lat), C.byref(out)) == 0
        assert abs(out.value - ref) <= 4e-14 * ref, (lat, out.value, ref)


@pytest.mark.parametrize("case,test", [("tc", 2), ("bw", 1)])
def test_fixtures_exercise_every_branch(case, test):
    """The moistened starting state makes every branch act (RJ supersaturation, Kessler precipitation, lowest-level wind on
    both sides of 20 m/s, presi and zi on both sides of pbltop and zpbltop, an interface inside the Bryan boundary layer where
    its diffusivity is not zero), and the fixtures tell the variants apart."""
    d = dc.load_case(case)
    for k, v in d.items():
        if k.startswith("branches/moist/"):
            assert int(v[0]) > 0, k
    def after(call, p, what):
        return dc.decode_after(d, "moist", call, p, what)
    for p in range(6):
        base = "moist_t%d_pbl%%d_prec%%d" % test
        assert not np.array_equal(after(base % (0, 0), p, "node"), after(base % (1, 0), p, "node"))
        assert not np.array_equal(after(base % (0, 0), p, "tracers"), after(base % (0, 1), p, "tracers"))
        # test 3 (supercell) skips the boundary layer: it differs from test `test` with the same precipitation
        assert not np.array_equal(after("moist_t3_pbl0_prec0", p, "node"), after(base % (0, 0), p, "node"))
    pr0 = sum(float(np.sum(d["prect/moist_t%d_pbl0_prec0/p%d" % (test, p)])) for p in range(6))
    pr1 = sum(float(np.sum(d["prect/moist_t%d_pbl0_prec1/p%d" % (test, p)])) for p in range(6))
    assert pr0 > 0.0 and pr1 > 0.0 and pr0 != pr1


def test_moist_baroclinic_wave_leaves_the_chemistry_tracers_alone():
    """BaroclinicWaveUMJSTest carries 5 tracers; DCMIPPhysics::Perform writes only the first three.  The generator checks
    tracers 3 and 4 bit for bit and leaves them out of the stored results: here the starting states carry them and they are
    not all zero, so the check was not vacuous."""
    d = dc.load_case("bw")
    for start in ("stock", "warm", "moist"):
        tr = d["state/%s/p0/tracers" % start]
        assert tr.shape[0] == 5 and np.any(tr[3:] != 0.0)
        assert d["xor/%s_t1_pbl0_prec0/p0/tracers" % start].shape[0] == 3
