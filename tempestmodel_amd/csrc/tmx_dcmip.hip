// tmx_dcmip.hip -- host side of the DCMIP2016 column physics: DCMIPPhysics::Perform (test/dcmip2016/DCMIPPhysics.cpp:156-409) around
// SUBROUTINE DCMIP2016_PHYSICS (test/dcmip2016/interface/dcmip_physics_z_v1.f90).  Set-up forms, per stored column, everything that
// only depends on the node's position with the host's libm, in the reference's expression order: the coefficients of the two
// covector transforms around the call and the test-1 surface temperature.  The kernel (tmx_k_physics.hip: k_dcmip) is left with
// products, sums and the exp / pow of the column.
#include "tmx_hostshared.h"

// CubedSphereTrans::CoVecTransRLLFromABP / CoVecTransABPFromRLL (src/atm/CubedSphereTrans.cpp:549-729) as coefficient x component
// products, out[TMX_DC_NCOEF] without the last entry:
//   u_lon = (RA0 * u_a + RA1 * u_b) * RCOS,  u_lat = RB0 * u_a + RB1 * u_b
//   l = u_lon / ADIV,  u_a = AA0 * l + AA1 * u_lat,  u_b = AB0 * l + AB1 * u_lat
// Every coefficient is the reference's left-to-right product / quotient chain up to the component it multiplies; a term the
// reference subtracts is added with its coefficient negated (a - b * c == a + (-b) * c in IEEE arithmetic); cos(lat) multiplies the
// longitude component of the first transform and divides it in the second, as there.  A coefficient of 0 stands for a term the
// reference does not have (0 * u + v == v up to the sign of a zero result).
static void dcmip_node_coefficients(int nP, double dX, double dY, double * o) {
	const double dDelta2 = 1.0 + dX * dX + dY * dY;
	if ((nP > 3) && (fabs(dX) < 1.0e-13) && (fabs(dY) < 1.0e-13)) {      // panel centres of the polar panels (:561-569, :644-652)
		const double s = (nP == 4) ? 1.0 : -1.0;
		o[DC_RA0] = s; o[DC_RA1] = 0.0; o[DC_RB0] = 0.0; o[DC_RB1] = 1.0; o[DC_RCOS] = 1.0;
		o[DC_ADIV] = 1.0; o[DC_AA0] = s; o[DC_AA1] = 0.0; o[DC_AB0] = 0.0; o[DC_AB1] = 1.0;
		return;
	}
	if (nP <= 3) {
		// RLL from ABP (:656-669)
		o[DC_RA0] = dDelta2 / (1.0 + dX * dX);
		o[DC_RA1] = dDelta2 * dX * dY / (1.0 + dX * dX) / (1.0 + dY * dY);
		o[DC_RB0] = 0.0;
		o[DC_RB1] = dDelta2 / sqrt(1.0 + dX * dX) / (1.0 + dY * dY);
		const double lat = atan(dY / sqrt(1.0 + dX * dX));
		o[DC_RCOS] = cos(lat);
		// ABP from RLL (:578-590)
		o[DC_ADIV] = cos(lat);
		o[DC_AA0] = (1.0 + dX * dX) / dDelta2;
		o[DC_AA1] = -(dX * dY * sqrt(1.0 + dX * dX) / dDelta2);
		o[DC_AB0] = 0.0;
		o[DC_AB1] = sqrt(1.0 + dX * dX) * (1.0 + dY * dY) / dDelta2;
		return;
	}
	const double dRadius2 = (dX * dX + dY * dY);
	const double dRadius = sqrt(dRadius2);
	const double sg = (nP == 4) ? 1.0 : -1.0;      // the south panel's terms are the north panel's with the signs flipped
	// RLL from ABP (:672-709); both polar panels take lat = pi/2 - atan(r) there
	o[DC_RA0] = -sg * (dDelta2 * dY / (1.0 + dX * dX) / dRadius2);
	o[DC_RA1] = sg * (dDelta2 * dX / (1.0 + dY * dY) / dRadius2);
	o[DC_RB0] = -sg * (dDelta2 * dX / (1.0 + dX * dX) / dRadius);
	o[DC_RB1] = -sg * (dDelta2 * dY / (1.0 + dY * dY) / dRadius);
	o[DC_RCOS] = cos(0.5 * M_PI - atan(sqrt(dX * dX + dY * dY)));
	// ABP from RLL (:593-630)
	const double lat = (nP == 4) ? 0.5 * M_PI - atan(sqrt(dX * dX + dY * dY)) : -0.5 * M_PI + atan(sqrt(dX * dX + dY * dY));
	o[DC_ADIV] = cos(lat);
	o[DC_AA0] = -sg * (dY * (1.0 + dX * dX) / dDelta2);
	o[DC_AA1] = -sg * (dX * (1.0 + dX * dX) / (dDelta2 * dRadius));
	o[DC_AB0] = sg * (dX * (1.0 + dY * dY) / dDelta2);
	o[DC_AB1] = -sg * (dY * (1.0 + dY * dY) / (dDelta2 * dRadius));
}

// Tsurf of test 1 (dcmip_physics_z_v1.f90:204-212) as the reference's Fortran build evaluates it (amdflang -O3, no FMA on the
// host): the constant sub-expressions are folded at compile time, (sin lat)**6 and (cos lat)**3 are chains of multiplications,
// (-2 s^6 (c^2 + 1/3) + 10/63) is 10/63 - 2 s^6 (c^2 + 1/3), -(lat/latw)**4 is q^3 * (-q).
static double dcmip_tsurf_test1(double lat) {
	const double third = 0x1.5555555555555p-2;          // 1/3
	const double two_thirds = 0x1.5555555555555p-1;     // 2/3
	const double m_pi_4 = -0x1.921fb54442d18p-1;        // -pi/4
	const double ten_63 = 0x1.4514514514514p-3;         // 10/63
	const double c_etav = 0x1.ea5a41484d163p-3;         // u0-term factor (cos(etav))**1.5
	const double c_tsurf = 0x1.5128a340d0862p-2;        // pi*u0/rair * 1.5 * sin(etav) * (cos(etav))**0.5
	const double latw = 0x1.657184ae74487p-1;           // 2 pi / 9
	const double zq = 0x1.a26433bfdcd5ap-7;             // zvir * q0
	const double s = sin(lat), s2 = s * s;
	const double s6 = s * (s * (s * (s * s2)));
	const double c = cos(lat), c2 = c * c, c3 = c * c2;
	const double t_u0 = (ten_63 - (c2 + third) * (s6 * 2.0)) * 35.0 * c_etav;
	const double t_om = ((s2 + two_thirds) * (c3 * 1.6) + m_pi_4) * 6371220.0 * 7.29212e-5 * 0.5;
	const double q = lat / latw, q3 = q * (q * q);
	return ((t_om + t_u0) * c_tsurf + 288.0) / (exp(q3 * (-q)) * zq + 1.0);
}

extern "C" int tmx_debug_dcmip_node_coefficients(int panel, double alpha, double beta, double * out) {
	REQUIRE(out && panel >= 0 && panel < 6, TMX_ERR_INVALID, "tmx_debug_dcmip_node_coefficients: panel in [0, 6) and out required");
	dcmip_node_coefficients(panel, tan(alpha), tan(beta), out);
	out[DC_TSURF1] = 0.0;
	return TMX_OK;
}

extern "C" int tmx_debug_dcmip_tsurf(double lat, double * out) {
	REQUIRE(out, TMX_ERR_INVALID, "tmx_debug_dcmip_tsurf: null argument");
	*out = dcmip_tsurf_test1(lat);
	return TMX_OK;
}

extern "C" int tmx_set_patch_dcmip_inputs(tmx_engine * e, int patch, const double * latitude, const double * a_nodes, const double * b_nodes,
	const double * z_interfaces, double earth_radius)
{
	REQUIRE(e && latitude && a_nodes && b_nodes && z_interfaces, TMX_ERR_INVALID, "tmx_set_patch_dcmip_inputs: null argument");
	REQUIRE(patch >= 0 && patch < e->cfg.n_patches, TMX_ERR_INVALID, "patch index out of range");
	REQUIRE(!e->sw, TMX_ERR_UNSUPPORTED, "column physics with the shallow-water equation set is not supported");
	REQUIRE(earth_radius > 0.0, TMX_ERR_INVALID, "tmx_set_patch_dcmip_inputs: earth_radius must be positive");
	REQUIRE(e->dcmip_radius == 0.0 || e->dcmip_radius == earth_radius, TMX_ERR_INVALID, "tmx_set_patch_dcmip_inputs: one earth_radius for all patches");
	int r = ensure_layout(e);
	if (r) return r;
	PatchInfo & P = e->patches[patch];
	REQUIRE(P.owner == e->cfg.rank, TMX_ERR_INVALID, "patch %d is not owned by rank %d", patch, e->cfg.rank);
	REQUIRE(P.panel >= 0 && P.panel < 6, TMX_ERR_INVALID, "patch %d has no panel", patch);
	const int L = e->L;
	const size_t NS = e->NS;
	if (e->h_dcmip.empty()) { e->h_dcmip.assign((size_t)TMX_DC_NCOEF * NS, 0.0); e->h_zint.assign((size_t)(L + 1) * NS, 0.0); }
	for (int i = 1; i < P.na - 1; i++)
	for (int j = 1; j < P.nb - 1; j++) {
		const int c = col_of(P, i, j);
		double o[TMX_DC_NCOEF];
		dcmip_node_coefficients(P.panel, tan(a_nodes[i]), tan(b_nodes[j]), o);      // DCMIPPhysics.cpp:272-279, :374-381
		o[DC_TSURF1] = dcmip_tsurf_test1(latitude[(size_t)i * P.nb + j]);
		for (int f = 0; f < TMX_DC_NCOEF; f++) e->h_dcmip[(size_t)f * NS + c] = o[f];
		for (int k = 0; k <= L; k++) e->h_zint[(size_t)k * NS + c] = z_interfaces[((size_t)i * P.nb + j) * (L + 1) + k];
	}
	e->dcmip_radius = earth_radius;
	P.dcmip_set = true; e->dcmip_dirty = true;
	return TMX_OK;
}

extern "C" int tmx_physics_dcmip2016(tmx_engine * e, int instance, double dt, int test, int pbl_type, int prec_type) {
	int r; if ((r = check_ready(e))) return r;
	REQUIRE(instance >= 0 && instance < e->cfg.n_instances, TMX_ERR_INVALID, "instance %d out of range [0,%d)", instance, e->cfg.n_instances);
	// (the engine keeps theta on levels, Lorenz staggering; the reference throws for theta on interfaces, DCMIPPhysics.cpp:180-182)
	REQUIRE(!e->sw, TMX_ERR_UNSUPPORTED, "DCMIP2016 physics with the shallow-water equation set is not supported");
	REQUIRE(e->nt >= 3, TMX_ERR_INVALID, "DCMIP2016 physics needs the tracers RhoQv, RhoQc, RhoQr (n_tracers >= 3)");
	REQUIRE(test >= 1 && test <= 3, TMX_ERR_INVALID, "tmx_physics_dcmip2016: test %d not in {1, 2, 3}", test);
	REQUIRE(pbl_type == 0 || pbl_type == 1, TMX_ERR_INVALID, "tmx_physics_dcmip2016: pbl_type %d not in {0, 1}", pbl_type);
	REQUIRE(prec_type == 0 || prec_type == 1, TMX_ERR_INVALID, "tmx_physics_dcmip2016: prec_type %d not in {0, 1}", prec_type);
	REQUIRE(dt > 0.0, TMX_ERR_INVALID, "tmx_physics_dcmip2016: dt must be positive");
	for (int lp : e->local_patches) {
		REQUIRE(e->patches[lp].zlev_set, TMX_ERR_INVALID, "tmx_set_patch_level_heights was not called for patch %d", lp);
		REQUIRE(e->patches[lp].dcmip_set, TMX_ERR_INVALID, "tmx_set_patch_dcmip_inputs was not called for patch %d", lp);
	}
	if ((r = check_inst(e, instance))) return r;      // a node-unique instance becomes element-major here, as for Kessler
	if ((r = column_physics_levels(e))) return r;
	const size_t NS = e->NS; const int L = e->L;
	if (!e->d_dcmip) {
		HIPCHK(hipMalloc((void **)&e->d_dcmip, (size_t)TMX_DC_NCOEF * NS * sizeof(double)));
		HIPCHK(hipMalloc((void **)&e->d_zint, (size_t)(L + 1) * NS * sizeof(double)));
		HIPCHK(hipMalloc((void **)&e->d_dcw, (size_t)TMX_DC_NW * L * NS * sizeof(double)));
		e->hbm_bytes += (size_t)(TMX_DC_NCOEF + L + 1 + TMX_DC_NW * L) * NS * sizeof(double);
	}
	if (e->dcmip_dirty) {
		HIPCHK(hipStreamSynchronize(e->stream));
		HIPCHK(hipMemcpy(e->d_dcmip, e->h_dcmip.data(), (size_t)TMX_DC_NCOEF * NS * sizeof(double), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(e->d_zint, e->h_zint.data(), (size_t)(L + 1) * NS * sizeof(double), hipMemcpyHostToDevice));
		e->dcmip_dirty = false;
	}
	// the Thomas coefficients in LDS hold a CU to one 64-column workgroup at L30 (92 KiB): 2.6 against 0.85 ms at ne30
	const bool lds = e->opt_dcmip_lds && tmxk_dcmip_lds_bytes(L) != 0;
	ProfScope ps(e, TMX_K_LINCOMB);
	tmxk_dcmip(e, make_params(e), inst(e, instance), dt, test, pbl_type, prec_type, e->dcmip_radius, lds);
	return launch_check("physics_dcmip2016");
}
