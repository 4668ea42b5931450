// tmx_program.hip -- host side of the engine, part 3: the time-stepper programs -- their builder, the matcher of fused units, the
// access analysis with the copy sharing it allows, and the element-major and node-unique interpreters behind tmx_step.  (The
// operations the interpreters launch: tmx_step.hip; shared declarations: tmx_hostshared.h.)
#include "tmx_hostshared.h"

// ARS(3,4,3) tableau in U-form (TimestepSchemeARS343.cpp:25-146)
static void ars343_tableau(double * u2, double * u3, double * u4, double * dexp, double * dimp) {
	const double gm = 0.4358665215084590;
	const double b1 = -1.5 * gm * gm + 4.0 * gm - 0.25;
	const double b2 = 1.5 * gm * gm - 5.0 * gm + 1.25;
	const double a42 = 0.5529291480359398, a43 = 0.5529291480359398;
	const double a31 = (1.0 - 4.5 * gm + 1.5 * gm * gm) * a42 + (2.75 - 10.5 * gm + 3.75 * gm * gm) * a43 - 3.5 + 13 * gm - 4.5 * gm * gm;
	const double a32 = (-1.0 + 4.5 * gm - 1.5 * gm * gm) * a42 + (-2.75 + 10.5 * gm - 3.75 * gm * gm) * a43 + 4.0 - 12.5 * gm + 4.5 * gm * gm;
	const double a41 = 1.0 - a42 - a43;
	const double I[4][4] = { { gm, 0, 0, 0 }, { 0.5 * (1.0 - gm), gm, 0, 0 }, { b1, b2, gm, 0 }, { b1, b2, gm, 0 } };
	const double E[4][4] = { { gm, 0, 0, 0 }, { a31, a32, 0, 0 }, { a41, a42, a43, 0 }, { 0, b1, b2, gm } };
	for (int i = 0; i < 4; i++) { dexp[i] = E[i][i]; dimp[i] = I[i][i]; }
	for (int i = 0; i < 7; i++) u2[i] = u3[i] = u4[i] = 0.0;
	u2[0] = 1.0 - E[1][0] / E[0][0]; u2[1] = E[1][0] / E[0][0] - I[1][0] / I[0][0]; u2[2] = I[1][0] / I[0][0];
	u3[0] = 1.0 - E[2][0] / E[0][0]; u3[1] = E[2][0] / E[0][0] - I[2][0] / I[0][0]; u3[2] = I[2][0] / I[0][0];
	u3[3] = E[2][1] / E[1][1] - I[2][1] / I[1][1]; u3[4] = I[2][1] / I[1][1];
	const double u37 = -E[2][1] / E[1][1];
	u4[0] = 1.0 - E[3][0] / E[0][0]; u4[1] = E[3][0] / E[0][0] - I[3][0] / I[0][0]; u4[2] = I[3][0] / I[0][0];
	u4[3] = E[3][1] / E[1][1] - I[3][1] / I[1][1]; u4[4] = I[3][1] / I[1][1];
	u4[5] = E[3][2] / E[2][2] - I[3][2] / I[2][2]; u4[6] = I[3][2] / I[2][2];
	const double u47 = -E[3][1] / E[1][1], u48 = -E[3][2] / E[2][2];
	u3[0] += u37 * u2[0]; u3[1] += u37 * u2[1]; u3[2] += u37 * u2[2];
	u4[0] += u47 * u2[0] + u48 * u3[0]; u4[1] += u47 * u2[1] + u48 * u3[1]; u4[2] += u47 * u2[2] + u48 * u3[2];
	u4[3] += u48 * u3[3]; u4[4] += u48 * u3[4];
}

// ---------------------------------------------------------------------------------------------
// Time steppers.  Every reference TimestepScheme::Step on this path is a fixed sequence of the same
// few Grid / HorizontalDynamics / VerticalDynamics calls; it is written down here call for call as a
// small program, and run_program folds neighbouring calls into one kernel pass where the result is
// bit-identical (see the rules there).

enum OpKind { OP_COPY, OP_LINCOMB, OP_HEXP, OP_VEXP, OP_DSS, OP_VIMP, OP_VITE, OP_HVIS, OP_VFILT };
struct Op {
	int kind, a, b, c;
	double coef;
	double lc[12];
	int nlc;
};
typedef std::vector<Op> Program;

static void P_copy(Program & p, int a, int b) { Op o = { OP_COPY, a, b, 0, 0.0, { 0 }, 0 }; p.push_back(o); }
static void P_h(Program & p, int i, int u, double c) { Op o = { OP_HEXP, i, u, 0, c, { 0 }, 0 }; p.push_back(o); }
static void P_v(Program & p, int i, int u, double c) { Op o = { OP_VEXP, i, u, 0, c, { 0 }, 0 }; p.push_back(o); }
static void P_hv(Program & p, int i, int u, double c) { P_h(p, i, u, c); P_v(p, i, u, c); }
static void P_dss(Program & p, int i) { Op o = { OP_DSS, i, 0, 0, 0.0, { 0 }, 0 }; p.push_back(o); }
static void P_vimp(Program & p, int i, int u, double c) { Op o = { OP_VIMP, i, u, 0, c, { 0 }, 0 }; p.push_back(o); }
static void P_vfilt(Program & p, int u) { Op o = { OP_VFILT, u, u, 0, 0.0, { 0 }, 0 }; p.push_back(o); }
static void P_vite(Program & p, int i, int u, double c) { Op o = { OP_VITE, i, u, 0, c, { 0 }, 0 }; p.push_back(o); }
static void P_hvis(Program & p, int i, int u, int w, double c) { Op o = { OP_HVIS, i, u, w, c, { 0 }, 0 }; p.push_back(o); }
static void P_lc(Program & p, const double * cf, int n, int dst) {
	Op o = { OP_LINCOMB, dst, 0, 0, 0.0, { 0 }, n };
	for (int i = 0; i < n; i++) o.lc[i] = cf[i];
	p.push_back(o);
}

// A fused unit: the operations from p[i] on that an interpreter may run as one.  match_unit recognises the STRUCTURE only (kinds, equal
// operands); each interpreter applies its own side conditions to the Unit it gets and, where it declines, runs p[i] on its own.
enum UnitKind {
	U_STAGE,          // [Copy(base -> upd) | LinearCombine(lc -> upd) | nothing: in place, base == upd]; H(init, upd, coef); V(init, upd, .)
	U_COPY_VIMP,      // Copy(base -> upd) [repeated]; V.StepImplicit(upd, upd, coef), base != upd
	U_COPY_HVIS,      // the Copy(base -> upd) in front of StepAfterSubCycle(base, upd, .), base != upd: the copy alone, which is dropped
	U_OP              // p[i] on its own
};
struct Unit {
	UnitKind kind;
	int n_ops;                       // operations of the unit, the DSS behind a stage not counted
	int init, base, upd; double coef;
	const double * lc; int nlc;      // stage: the combination it starts from, or null
	bool from_copy, same_coef;       // stage: it starts from a Copy; H and V carry the same coefficient
	bool dss_follows;                // stage: the next operation is DSS(upd)
};
static Unit match_unit(const Program & p, size_t i) {
	const size_t n = p.size();
	const Op & o = p[i];
	Unit u = { U_OP, 1, -1, -1, -1, 0.0, nullptr, 0, false, false, false };
	if (o.kind == OP_COPY || o.kind == OP_LINCOMB || o.kind == OP_HEXP) {
		const size_t h = i + (o.kind == OP_HEXP ? 0 : 1);      // where the stage's H stands
		const int upd = o.kind == OP_LINCOMB ? o.a : o.b;
		if (h + 1 < n && p[h].kind == OP_HEXP && p[h + 1].kind == OP_VEXP && p[h].b == upd && p[h + 1].b == upd && p[h + 1].a == p[h].a) {
			u.kind = U_STAGE; u.n_ops = (int)(h + 2 - i);
			u.init = p[h].a; u.upd = upd; u.coef = p[h].coef; u.same_coef = p[h].coef == p[h + 1].coef;
			u.from_copy = o.kind == OP_COPY; u.base = u.from_copy ? o.a : upd;
			if (o.kind == OP_LINCOMB) { u.lc = o.lc; u.nlc = o.nlc; }
			u.dss_follows = h + 2 < n && p[h + 2].kind == OP_DSS && p[h + 2].a == upd;
			return u;
		}
	}
	if (o.kind == OP_COPY && o.a != o.b) {
		size_t j = i + 1;
		while (j < n && p[j].kind == OP_COPY && p[j].a == o.a && p[j].b == o.b) j++;
		if (j < n && p[j].kind == OP_VIMP && p[j].a == o.b && p[j].b == o.b) { u.kind = U_COPY_VIMP; u.n_ops = (int)(j + 1 - i); u.coef = p[j].coef; }
		else if (j == i + 1 && j < n && p[j].kind == OP_HVIS && p[j].a == o.a && p[j].b == o.b) u.kind = U_COPY_HVIS;
		if (u.kind != U_OP) { u.base = o.a; u.upd = o.b; }
	}
	return u;
}

static int scheme_instances(int scheme) {
	switch (scheme) {
		case TMX_SCHEME_ARS343: return 7;    // TimestepSchemeARS343.h:48-56
		case TMX_SCHEME_ARS232: return 7;    // TimestepSchemeARS232.h
		case TMX_SCHEME_ARS222: return 4;
		case TMX_SCHEME_ARS443: return 10;
		case TMX_SCHEME_ARK232: return 8;
		case TMX_SCHEME_STRANG: case TMX_SCHEME_STRANG_FE: case TMX_SCHEME_STRANG_RK4: case TMX_SCHEME_STRANG_SSP3:
		case TMX_SCHEME_STRANG_SSPRK53: return 5;    // TimestepSchemeStrang.h GetComponentDataInstances
	}
	return -1;
}

// U-form combination coefficients shared by the ARS schemes: u_f(stage) from explicit/implicit tableaux
static int build_program(int scheme, int first, int last, double dt, Program & p, double offc = 0.0) {
	p.clear();
	if (scheme == TMX_SCHEME_ARS343) {
		// TimestepSchemeARS343::Step (TimestepSchemeARS343.cpp:150-236)
		double u2[7], u3[7], u4[7], de[4], di[4];
		ars343_tableau(u2, u3, u4, de, di);
		P_copy(p, 0, 1); P_hv(p, 0, 1, de[0] * dt); P_dss(p, 1);
		P_copy(p, 1, 2); P_vimp(p, 2, 2, di[0] * dt);
		P_lc(p, u2, 7, 3); P_hv(p, 2, 3, de[1] * dt); P_dss(p, 3);
		P_copy(p, 3, 4); P_vimp(p, 4, 4, di[1] * dt);
		P_lc(p, u3, 7, 5); P_hv(p, 4, 5, de[2] * dt); P_dss(p, 5);
		P_copy(p, 5, 6); P_vimp(p, 6, 6, di[2] * dt);
		P_lc(p, u4, 7, 1); P_hv(p, 6, 1, de[3] * dt); P_dss(p, 1);
		P_copy(p, 1, 0); P_hvis(p, 1, 0, 2, dt);
		return TMX_OK;
	}
	if (scheme == TMX_SCHEME_ARS232) {
		// TimestepSchemeARS232::Step (TimestepSchemeARS232.cpp:25-150)
		const double g = 1.0 - 1.0 / std::sqrt(2.0), d = -(2.0 * std::sqrt(2.0)) / 3.0;
		const double I[3][3] = { { g, 0, 0 }, { 1.0 - g, g, 0 }, { 1.0 - g, g, 0 } };
		const double E[3][3] = { { g, 0, 0 }, { d, 1.0 - d, 0 }, { 0, 1.0 - g, g } };
		double u2[6] = { 1.0 - E[1][0] / E[0][0], E[1][0] / E[0][0] - I[1][0] / I[0][0], I[1][0] / I[0][0], 0, 0, 0 };
		double u3[7] = { 1.0 - E[2][0] / E[0][0], E[2][0] / E[0][0] - I[2][0] / I[0][0], I[2][0] / I[0][0],
			E[2][1] / E[1][1] - I[2][1] / I[1][1], I[2][1] / I[1][1], -E[2][1] / E[1][1], 0 };
		P_copy(p, 0, 1); P_hv(p, 0, 1, E[0][0] * dt); P_dss(p, 1);
		P_copy(p, 1, 2); P_vimp(p, 2, 2, I[0][0] * dt);
		P_lc(p, u2, 6, 5); P_copy(p, 5, 3); P_hv(p, 2, 3, E[1][1] * dt); P_dss(p, 3);
		P_copy(p, 3, 4); P_vimp(p, 4, 4, I[1][1] * dt);
		P_lc(p, u3, 7, 6); P_hv(p, 4, 6, E[2][2] * dt); P_dss(p, 6);
		P_copy(p, 6, 2); P_hvis(p, 2, 1, 6, dt); P_copy(p, 1, 0);
		return TMX_OK;
	}
	if (scheme == TMX_SCHEME_ARS222) {
		// TimestepSchemeARS222::Step (TimestepSchemeARS222.cpp:25-119)
		const double g = 1.0 - 0.5 * std::sqrt(2.0), d = 1.0 - 1.0 / (2.0 * g);
		const double I[2][2] = { { g, 0 }, { 1.0 - g, g } };
		const double E[2][2] = { { g, 0 }, { d, 1.0 - d } };
		double u2[4] = { 1.0 - E[1][0] / E[0][0], E[1][0] / E[0][0] - I[1][0] / I[0][0], I[1][0] / I[0][0], 0 };
		P_copy(p, 0, 1); P_hv(p, 0, 1, E[0][0] * dt); P_dss(p, 1);
		P_copy(p, 1, 2); P_vimp(p, 2, 2, I[0][0] * dt); P_dss(p, 2);
		P_lc(p, u2, 4, 3); P_hv(p, 2, 3, E[1][1] * dt); P_dss(p, 3);
		P_vimp(p, 3, 3, I[1][1] * dt); P_dss(p, 3);
		P_copy(p, 3, 2); P_hvis(p, 2, 1, 3, dt); P_copy(p, 1, 0);
		return TMX_OK;
	}
	if (scheme == TMX_SCHEME_STRANG || (scheme >= TMX_SCHEME_STRANG_FE && scheme <= TMX_SCHEME_STRANG_SSPRK53)) {
		// TimestepSchemeStrang::Step (TimestepSchemeStrang.cpp:450-674) with each of its explicit discretisations
		// (:39-51, combinations :53-117) and the off-centering of its constructor
		const double half = 0.5 * dt, oc = offc;
		const double carry[2] = { 1.0, 1.0 }, offcomb[2] = { (2.0 - oc) / 2.0, oc / 2.0 }, fin[2] = { 1.0, -1.0 };
		if (first) P_vimp(p, 0, 0, half); else { P_lc(p, carry, 2, 0); P_vfilt(p, 0); }      // FilterNegativeTracers(0), :476-481
		if (scheme == TMX_SCHEME_STRANG_FE) {
			P_copy(p, 0, 4); P_hv(p, 0, 4, dt); P_dss(p, 4);
		} else if (scheme == TMX_SCHEME_STRANG_RK4) {
			const double rk4[5] = { -1.0 / 3.0, 1.0 / 3.0, 2.0 / 3.0, 1.0 / 3.0, 0.0 };
			P_copy(p, 0, 1); P_hv(p, 0, 1, half); P_dss(p, 1);
			P_copy(p, 0, 2); P_hv(p, 1, 2, half); P_dss(p, 2);
			P_copy(p, 0, 3); P_hv(p, 2, 3, dt); P_dss(p, 3);
			P_lc(p, rk4, 5, 4); P_hv(p, 3, 4, dt / 6.0); P_dss(p, 4);
		} else if (scheme == TMX_SCHEME_STRANG_SSP3) {
			const double a[3] = { 3.0 / 4.0, 1.0 / 4.0, 0.0 }, b[5] = { 1.0 / 3.0, 0.0, 2.0 / 3.0, 0.0, 0.0 };
			P_copy(p, 0, 1); P_hv(p, 0, 1, dt); P_dss(p, 1);
			P_lc(p, a, 3, 2); P_hv(p, 1, 2, 0.25 * dt); P_dss(p, 2);
			P_lc(p, b, 5, 4); P_hv(p, 2, 4, (2.0 / 3.0) * dt); P_dss(p, 4);
		} else if (scheme == TMX_SCHEME_STRANG_SSPRK53) {
			const double a[4] = { 0.355909775063327, 0.0, 0.644090224936674, 0.0 };
			const double b[4] = { 0.367933791638137, 0.0, 0.0, 0.632066208361863 };
			const double c[5] = { 0.762406163401431, 0.0, 0.237593836598569, 0.0, 0.0 };
			P_copy(p, 0, 1); P_hv(p, 0, 1, 0.377268915331368 * dt); P_dss(p, 1);
			P_copy(p, 1, 2); P_hv(p, 1, 2, 0.377268915331368 * dt); P_dss(p, 2);
			P_lc(p, a, 4, 3); P_hv(p, 2, 3, 0.242995220537396 * dt); P_dss(p, 3);
			P_lc(p, b, 4, 0); P_hv(p, 3, 0, 0.238458932846290 * dt); P_dss(p, 0);
			P_lc(p, c, 5, 4); P_hv(p, 0, 4, 0.287632146308408 * dt); P_dss(p, 4);
		} else {
			const double kgu[5] = { -1.0 / 4.0, 5.0 / 4.0, 0.0, 0.0, 0.0 };
			P_copy(p, 0, 1); P_hv(p, 0, 1, dt / 5.0); P_dss(p, 1);
			P_copy(p, 0, 2); P_hv(p, 1, 2, dt / 5.0); P_dss(p, 2);
			P_copy(p, 0, 3); P_hv(p, 2, 3, dt / 3.0); P_dss(p, 3);
			P_copy(p, 0, 2); P_hv(p, 3, 2, 2.0 * dt / 3.0); P_dss(p, 2);
			P_lc(p, kgu, 5, 4); P_hv(p, 2, 4, 3.0 * dt / 4.0); P_dss(p, 4);
		}
		P_copy(p, 4, 1); P_hvis(p, 4, 1, 2, dt);
		P_copy(p, 1, 0); P_vimp(p, 0, 0, 0.5 * (1.0 + oc) * dt);
		P_lc(p, offcomb, 2, 0);
		if (!last) P_lc(p, fin, 2, 1);
		return TMX_OK;
	}
	if (scheme == TMX_SCHEME_ARK232) {
		// TimestepSchemeARK232::Step with its two sub-cycled stages (TimestepSchemeARK232.cpp:25-225)
		const double g = 1.0 - 1.0 / std::sqrt(2.0), d = 1.0 / (2.0 * std::sqrt(2.0));
		const double al = 1.0 / 6.0 * (3.0 + 2.0 * std::sqrt(2.0));
		const double I[3][3] = { { g, g, 0 }, { d, d, g }, { d, d, g } };
		const double E[3][3] = { { 2.0 * g, 0, 0 }, { 1.0 - al, al, 0 }, { d, d, g } };
		double u2[7] = { 1.0 - E[1][0] / E[0][0], E[1][0] / E[0][0] - I[1][0] / I[0][0],
			I[1][0] / I[0][0] - I[1][1] / I[0][1], I[1][1] / I[0][1], 0, 0, 0 };
		double u3[8] = { 1.0 - E[2][0] / E[0][0], E[2][0] / E[0][0] - I[2][0] / I[0][0],
			I[2][0] / I[0][0] - I[2][1] / I[0][1], I[2][1] / I[0][1],
			E[2][1] / E[1][1] - I[2][2] / I[1][2], I[2][2] / I[1][2], -E[2][1] / E[1][1], 0 };
		// SubcycleStageExplicit(coeff E00, 2 sub-steps, 0 -> 1)
		for (int n = 0; n < 2; n++) {
			P_copy(p, 0, 1); P_hv(p, 0, 1, E[0][0] * dt / 2); P_dss(p, 1);
			if (n < 1) P_copy(p, 1, 0);
		}
		// SubcycleStageImplicitExplicitly(coeff I00, 1 sub-step, 1 -> 2)
		P_copy(p, 1, 2); P_vite(p, 1, 2, I[0][0] * dt); P_dss(p, 2);
		P_copy(p, 2, 3); P_vimp(p, 3, 3, I[0][1] * dt); P_dss(p, 3);
		P_lc(p, u2, 7, 6); P_copy(p, 6, 4); P_hv(p, 3, 4, E[1][1] * dt); P_dss(p, 4);
		P_copy(p, 4, 5); P_vimp(p, 5, 5, I[1][2] * dt); P_dss(p, 5);
		P_lc(p, u3, 8, 7); P_hv(p, 5, 7, E[2][2] * dt); P_dss(p, 7);
		P_copy(p, 7, 2); P_hvis(p, 7, 1, 3, dt); P_copy(p, 1, 0);
		return TMX_OK;
	}
	if (scheme == TMX_SCHEME_ARS443) {
		// TimestepSchemeARS443::Step (TimestepSchemeARS443.cpp)
		const double I[4][4] = { { 0.5, 0, 0, 0 }, { 1.0 / 6.0, 0.5, 0, 0 }, { -0.5, 0.5, 0.5, 0 }, { 1.5, -1.5, 0.5, 0.5 } };
		const double E[4][4] = { { 0.5, 0, 0, 0 }, { 11.0 / 18.0, 1.0 / 18.0, 0, 0 }, { 5.0 / 6.0, -5.0 / 6.0, 0.5, 0 }, { 0.25, 1.75, 0.75, -1.75 } };
		double u2[8], u3[9], u4[10];
		for (int i = 0; i < 8; i++) u2[i] = 0; for (int i = 0; i < 9; i++) u3[i] = 0; for (int i = 0; i < 10; i++) u4[i] = 0;
		u2[0] = 1.0 - E[1][0] / E[0][0]; u2[1] = E[1][0] / E[0][0] - I[1][0] / I[0][0]; u2[2] = I[1][0] / I[0][0];
		u3[0] = 1.0 - E[2][0] / E[0][0]; u3[1] = E[2][0] / E[0][0] - I[2][0] / I[0][0]; u3[2] = I[2][0] / I[0][0];
		u3[3] = E[2][1] / E[1][1] - I[2][1] / I[1][1]; u3[4] = I[2][1] / I[1][1]; u3[7] = -E[2][1] / E[1][1];
		u4[0] = 1.0 - E[3][0] / E[0][0]; u4[1] = E[3][0] / E[0][0] - I[3][0] / I[0][0]; u4[2] = I[3][0] / I[0][0];
		u4[3] = E[3][1] / E[1][1] - I[3][1] / I[1][1]; u4[4] = I[3][1] / I[1][1];
		u4[5] = E[3][2] / E[2][2] - I[3][2] / I[2][2]; u4[6] = I[3][2] / I[2][2];
		u4[7] = -E[3][1] / E[1][1]; u4[8] = -E[3][2] / E[2][2];
		P_copy(p, 0, 1); P_hv(p, 0, 1, E[0][0] * dt); P_dss(p, 1);
		P_copy(p, 1, 2); P_vimp(p, 2, 2, I[0][0] * dt); P_dss(p, 2);
		P_lc(p, u2, 8, 7); P_copy(p, 7, 3); P_hv(p, 2, 3, E[1][1] * dt); P_dss(p, 3);
		P_copy(p, 3, 4); P_vimp(p, 4, 4, I[1][1] * dt); P_dss(p, 4);
		P_lc(p, u3, 9, 8); P_copy(p, 8, 5); P_hv(p, 4, 5, E[2][2] * dt); P_dss(p, 5);
		P_copy(p, 5, 6); P_vimp(p, 6, 6, I[2][2] * dt); P_dss(p, 6);
		P_lc(p, u4, 10, 9); P_hv(p, 6, 9, E[3][3] * dt); P_dss(p, 9);
		P_vimp(p, 9, 9, I[3][3] * dt); P_dss(p, 9);
		P_copy(p, 9, 2); P_hvis(p, 2, 1, 9, dt); P_copy(p, 1, 0);
		return TMX_OK;
	}
	tmx_set_error("unknown time scheme %d", scheme);
	return TMX_ERR_INVALID;
}

// ---------------------------------------------------------------------------------------------
// access analysis and copy sharing

// What the analysis depends on beside the program.  vimp_noop: V.StepImplicit does nothing (fully explicit vertical mode, shallow
// water's stub); hvis_two_pass: StepAfterSubCycle writes its working instance (order-4 hyperviscosity with a non-zero coefficient);
// dry_unsafe: tmx_debug_program_copies' negative control (dry runs only) -- every share accepted, no copy-on-write
struct Access { bool vimp_noop, hvis_two_pass, dry_unsafe; };
// What an operation of a stepper program reads and writes, as bit masks over the data instances.  full: instances it
// overwrites entirely without reading them; part: instances it updates in place.
struct OpAccess { unsigned reads, full, part; bool stencil; };
static OpAccess op_access(const Op & o, Access ax) {
	OpAccess x = { 0u, 0u, 0u, true };
	auto bit = [](int k) { return 1u << k; };
	switch (o.kind) {
	case OP_COPY: x.reads = bit(o.a); x.full = bit(o.b); break;
	case OP_VIMP: if (ax.vimp_noop) break;      // fall through
	case OP_HEXP: case OP_VEXP: case OP_VITE: x.reads = bit(o.a) | bit(o.b); x.part = bit(o.b); break;
	case OP_DSS: case OP_VFILT: x.reads = bit(o.a); x.part = bit(o.a); break;
	// StepAfterSubCycle rewrites all of b on every branch; the working instance c is written (entirely) by the two-pass
	// branch only -- without viscosity or with one pass it is left alone, so a c that shares a slot keeps its contents
	case OP_HVIS: x.reads = bit(o.a); x.full = bit(o.b) | (ax.hvis_two_pass ? bit(o.c) : 0u); break;
	case OP_LINCOMB:
		x.stencil = false;      // node by node: a source may share the destination's slot
		for (int m = 0; m < o.nlc; m++) if (o.lc[m] != 0.0) x.reads |= bit(m);
		if (o.lc[o.a] != 0.0) x.part = bit(o.a); else x.full = bit(o.a);
		break;
	}
	return x;
}

// May instance b read instance a's slot from operation `first` of the program on, in place of a copy of a made just before?
// Yes if, until b is next overwritten entirely, nothing updates b in place, and once a has been written b is not read again
// (b is dead from there on); a stencil operation must not write a while it reads b.  A program that ends with the two still
// identical leaves them shared; one that ends after a was written would leave b undefined, so it is refused.
static bool share_is_safe(const Program & p, size_t first, int a, int b, Access ax) {
	if (ax.dry_unsafe) return true;
	const unsigned ba = 1u << a, bb = 1u << b;
	bool a_written = false;
	for (size_t i = first; i < p.size(); i++) {
		const OpAccess x = op_access(p[i], ax);
		if (x.part & bb) return false;
		if ((x.reads & bb) && a_written) return false;
		if (((x.full | x.part) & ba) && (x.reads & bb) && x.stencil) return false;
		if (x.full & bb) return true;
		if ((x.full | x.part) & ba) a_written = true;
	}
	return !a_written;
}

// an operation is about to write instance x: give it its own slot back (with its contents unless the write is total); the
// same for U,V slabs it shares
static int own_slot(tmx_engine * e, int x, bool total, Access ax) {
	if (e->imap[x] != x) {
		if (!total) {
			if (e->dry_run) { e->dry_copies++; if (!ax.dry_unsafe) for (int c = 0; c < 2; c++) e->dry_slot[c][x] = e->dry_slot[c][e->imap[x]]; }
			else HIPCHK(hipMemcpyAsync(e->d_state + (size_t)x * e->inst_stride, e->d_state + (size_t)e->imap[x] * e->inst_stride,
				e->inst_stride * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
		}
		e->imap[x] = x; e->n_shared--;
	}
	if (e->uvmap[x] != x) {
		if (!total) {
			if (e->dry_run) { e->dry_copies++; if (!ax.dry_unsafe) e->dry_slot[0][x] = e->dry_slot[0][e->uvmap[x]]; }
			else HIPCHK(hipMemcpyAsync(e->d_state + (size_t)x * e->inst_stride, e->d_state + (size_t)e->uvmap[x] * e->inst_stride,
				(size_t)2 * e->L * e->NS * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
		}
		e->uvmap[x] = x; e->n_uvshared--;
	}
	return TMX_OK;
}

struct ProgramScope {
	tmx_engine * e;
	ProgramScope(tmx_engine * e_) : e(e_) { e->in_program = true; }
	~ProgramScope() { e->in_program = false; }
};
struct AfterOp {      // at the end of an operation: the readers of the slots it wrote
	tmx_engine * e; unsigned w;
	~AfterOp() { for (int x = 0; x < (int)e->imap.size() && (e->n_shared || e->n_uvshared); x++) if (w >> x & 1u) drop_readers(e, x); }
};

// Symbolic model of the dry run.  Value ids stand for array contents: the reference's semantics of every operation is applied to
// dry_ref (per instance, U,V and the rest apart -- the implicit column solve is the one operation that writes only the rest),
// and an executed operation is taken to store the reference's result in the slots of the instances it writes, provided that
// every instance it read was found, through the instance maps, in a slot holding the reference's value: that is what is checked.
static unsigned long long dry_mix(unsigned long long h, unsigned long long v) { h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2); return h * 0xff51afd7ed558ccdull; }
static int dry_slot_of(const tmx_engine * e, int k, int c) { return (c == 0 && e->uvmap[k] != k) ? e->uvmap[k] : e->imap[k]; }
// operations [i0, i0 + n_ops) of the program were executed as one unit
static void dry_model(tmx_engine * e, const Program & p, size_t i0, size_t n_ops, Access ax) {
	const int ni = (int)e->imap.size();
	unsigned written[2] = { 0u, 0u };
	for (size_t j = i0; j < i0 + n_ops && j < p.size(); j++) {
		const Op & o = p[j];
		if (o.kind == OP_VIMP && ax.vimp_noop) continue;
		const OpAccess x = op_access(o, ax);
		const bool rest_only = (o.kind == OP_VIMP);            // V.StepImplicit leaves U,V alone
		// reads from outside the unit must find the reference's value where the maps point
		for (int k = 0; k < ni; k++)
			for (int c = 0; c < 2; c++)
				if ((x.reads >> k & 1u) && !(written[c] >> k & 1u) && e->dry_slot[c][dry_slot_of(e, k, c)] != e->dry_ref[c][k]) e->dry_mismatch++;
		// the reference's result
		std::vector<unsigned long long> nr[2] = { e->dry_ref[0], e->dry_ref[1] };
		for (int c = (rest_only ? 1 : 0); c < 2; c++) {
			auto in = [&](int k) { return dry_mix(e->dry_ref[0][k], e->dry_ref[1][k]); };      // a stencil operation's result depends on all of its input instance
			switch (o.kind) {
			case OP_COPY: nr[c][o.b] = e->dry_ref[c][o.a]; break;
			case OP_HEXP: case OP_VEXP: case OP_VITE: case OP_VIMP: nr[c][o.b] = dry_mix(dry_mix(dry_mix(1000 + o.kind, c), in(o.a)), e->dry_ref[c][o.b]); break;
			case OP_DSS: case OP_VFILT: nr[c][o.a] = dry_mix(dry_mix(2000 + o.kind, c), e->dry_ref[c][o.a]); break;
			case OP_HVIS: nr[c][o.b] = dry_mix(dry_mix(3000, c), in(o.a)); nr[c][o.c] = dry_mix(dry_mix(3001, c), in(o.a)); break;
			case OP_LINCOMB: {
				unsigned long long h = dry_mix(4000, c);
				for (int m = 0; m < o.nlc; m++) if (o.lc[m] != 0.0) { unsigned long long b; memcpy(&b, &o.lc[m], 8); h = dry_mix(dry_mix(h, b), e->dry_ref[c][m]); }
				nr[c][o.a] = h; break; }
			}
			written[c] |= x.full | x.part;
		}
		e->dry_ref[0] = nr[0]; e->dry_ref[1] = nr[1];
	}
	// the unit's results land in the slots of the instances it wrote (or must already be there, for an instance left sharing)
	for (int k = 0; k < ni; k++)
		for (int c = 0; c < 2; c++)
			if (written[c] >> k & 1u) {
				const int sl = dry_slot_of(e, k, c);
				if (sl == k) e->dry_slot[c][k] = e->dry_ref[c][k];
				else if (e->dry_slot[c][sl] != e->dry_ref[c][k]) e->dry_mismatch++;
			}
}

// RUN: the launches of an operation; a dry run (tmx_debug_program_copies: the copy / sharing decisions of a program on the
// host, no device) skips them
#define RUN(call) (e->dry_run ? TMX_OK : (call))

// An explicit stage on the element-major layout.  *ops: the operations consumed -- the DSS too where the stage runs boundary tiles first,
// exchange overlapped with the interior tiles (several ranks) -- or 0 where this layout declines the unit: its first operation runs alone.
static int run_stage(tmx_engine * e, const Unit & u, size_t * ops) {
	*ops = 0;
	const bool split = stage_can_split(e) && u.dss_follows;
	if (!e->sw) {
		// [Copy(a->b) | LinearCombine(-> b)] + H(i,b,c) + V(i,b,c)  ==  one pass  b = [a | combination] + c * rhs(i), the combination
		// evaluated inside the explicit kernels; H + V alone: b += c * rhs(i)
		if (!u.same_coef || ((u.from_copy || u.lc) && u.init == u.upd)) return TMX_OK;
		*ops = u.n_ops + (split ? 1 : 0);
		return RUN(hv_stage(e, u.init, u.base, u.upd, u.coef, u.lc, u.nlc, split));
	}
	// shallow water, no tracers: Copy(a->b) + H(i,b,c) [+ V stub]: out = a + c * rhs(i) in one pass (k_sw_explicit takes the base
	// apart); H [+ V stub] in place only as a boundary-first stage (otherwise H's own launch is all there is)
	if (u.lc || u.init == u.upd || (u.from_copy ? (e->nt != 0 || u.base == u.upd) : !split)) return TMX_OK;
	*ops = u.n_ops + (split ? 1 : 0);
	return RUN(sw_stage(e, u.init, u.base, u.upd, u.coef, split));
}

// dry_unsafe: see Access
static int run_program(tmx_engine * e, const Program & p, bool dry_unsafe = false) {
	int r;
	ProgramScope scope(e);
	const bool noop = e->sw || e->fully_explicit;      // V.StepImplicit does nothing
	const Access ax = { noop, e->dry_run || (hypervis_active(e) && e->cfg.hypervis_order != 2), dry_unsafe };
	// shared slots left by the previous step: kept where this program allows it, given their own copy otherwise
	for (int b = 0; b < (int)e->imap.size() && (e->n_shared || e->n_uvshared); b++)
		if ((e->imap[b] != b && !share_is_safe(p, 0, e->imap[b], b, ax)) || (e->uvmap[b] != b && !share_is_safe(p, 0, e->uvmap[b], b, ax)))
			if ((r = own_slot(e, b, false, ax))) return r;
	for (size_t i = 0, ops = 0; i < p.size(); i += ops) {
		const Op & o = p[i];
		const Unit u = match_unit(p, i);
		// the instances this operation (and the ones fused with it below, which write the same instance) writes
		const OpAccess acc = op_access(o, ax);
		for (int x = 0; x < (int)e->imap.size() && (e->n_shared || e->n_uvshared); x++)
			if (((acc.full | acc.part) >> x & 1u) && (r = own_slot(e, x, (acc.full >> x & 1u) != 0, ax))) return r;
		AfterOp after = { e, acc.full | acc.part };
		// the rules in the order they are tried; a unit that a rule declines (ops stays 0) runs its first operation on its own
		ops = 0;
		if (u.kind == U_STAGE) {
			if ((r = run_stage(e, u, &ops))) return r;
		} else if (u.kind == U_COPY_VIMP && !noop) {
			// Copy(s->t) [twice in some schemes] + V.StepImplicit(t,t,c): the solve rewrites rho*theta, W, rho
			// of every stored column, so only U,V need copying and the solve reads s directly
			// ... and U,V need not be copied either while the copy's U,V are only read by the fused explicit stage
			// (k_h_explicit takes the U,V slabs of its initial instance and of the combination sources by separate
			// pointers, k_h_tracers those of its initial instance): the copy shares its source's U,V slabs under the rules
			// of share_is_safe.
			const bool share = e->share_copies && !e->use_graph && e->imap[u.base] == u.base && e->uvmap[u.base] == u.base &&
				share_is_safe(p, i + u.n_ops, u.base, u.upd, ax);
			if (share) { if ((r = RUN(surface_copy(e, u.base, u.upd)))) return r; }
			else { if (e->dry_run) e->dry_copies++; if ((r = RUN(copy_uv(e, u.base, u.upd)))) return r; }
			if ((r = RUN(v_step_implicit_impl(e, u.base, u.upd, u.coef, u.base)))) return r;
			if (share) {
				drop_readers(e, u.upd);
				e->uvmap[u.upd] = u.base; e->n_uvshared++; e->dry_shared++;
				after.w = 0;
			}
			ops = u.n_ops;
		} else if (u.kind == U_COPY_HVIS) {
			// Copy(a->b) + StepAfterSubCycle(a,b,w): every branch of StepAfterSubCycle rewrites all of b from a (the second
			// hyperviscosity pass and the order-2 pass write every slab with a as their base; without viscosity it IS the copy)
			ops = 1;
		}
		if (!ops) {
			ops = 1;
			switch (o.kind) {
			case OP_COPY:
				// Any other Copy(a->b) whose copy is only read until it is next overwritten entirely (share_is_safe) is not made: b
				// reads a's slot.  The case that matters: the copies in front of a V.StepImplicit that does nothing (fully explicit
				// vertical mode :1239-1242, shallow water's stub) -- config 4: three whole-state copies per ARS343 step.
				// (not into instance 0: the model state, which everything outside a step reads)
				if (e->share_copies && !e->use_graph && o.a != o.b && o.b != 0 && e->imap[o.a] == o.a && e->uvmap[o.a] == o.a && share_is_safe(p, i + 1, o.a, o.b, ax)) {
					drop_readers(e, o.b);      // (dead by the same argument: b is overwritten here)
					e->imap[o.b] = o.a; e->n_shared++; e->dry_shared++;
					after.w = 0;
				} else if (e->dry_run) e->dry_copies++;
				else if ((r = tmx_copy_data(e, o.a, o.b))) return r;
				break;
			case OP_LINCOMB: if ((r = RUN(tmx_linear_combine_data(e, o.lc, o.nlc, o.a)))) return r; break;
			case OP_HEXP: if ((r = RUN(tmx_h_step_explicit(e, o.a, o.b, o.coef)))) return r; break;
			case OP_VEXP: if ((r = RUN(tmx_v_step_explicit(e, o.a, o.b, o.coef)))) return r; break;
			case OP_DSS: if ((r = RUN(tmx_apply_dss(e, o.a)))) return r; break;
			case OP_VIMP: if ((r = RUN(tmx_v_step_implicit(e, o.a, o.b, o.coef)))) return r; break;
			case OP_VFILT: if ((r = RUN(tmx_v_filter_negative_tracers(e, o.a)))) return r; break;      // nothing without tracers
			case OP_VITE: if ((r = RUN(tmx_v_step_implicit_terms_explicitly(e, o.a, o.b, o.coef)))) return r; break;
			case OP_HVIS: if ((r = RUN(h_step_after_subcycle_impl(e, o.a, o.b, o.c, o.coef, true)))) return r; break;
			}
		}
		if (e->dry_run) dry_model(e, p, i, ops, ax);      // (before `after` drops the readers of the slots the unit wrote)
	}
	return TMX_OK;
}

#undef RUN

// The instance copies a stepper program performs (whole instances; with implicit vertical dynamics the U,V slabs in front of
// the column solve) and the ones it replaces by slot sharing, decided exactly as
// run_program decides them, without a device: `steps` consecutive steps (the first with first_step set), counts of the last
// one.  mode 0: implicit vertical dynamics, 1: fully explicit vertical mode, 2: shallow water.  Host logic for the CPU tests.
extern "C" int tmx_debug_program_copies(int scheme, int mode, int steps, int share, int * copies, int * shared) {
	REQUIRE(copies && shared && steps >= 1 && mode >= 0 && mode <= 2, TMX_ERR_INVALID, "tmx_debug_program_copies: bad argument");
	const int need = scheme_instances(scheme);
	REQUIRE(need > 0, TMX_ERR_INVALID, "unknown time scheme %d", scheme);
	tmx_engine e;
	e.cfg.n_instances = need; e.cfg.n_ranks = 1;
	e.sw = mode == 2; e.fully_explicit = mode == 1; e.share_copies = share != 0; e.dry_run = true;
	e.imap.resize(need);
	for (int k = 0; k < need; k++) e.imap[k] = k;
	e.uvmap = e.imap;
	for (int c = 0; c < 2; c++) {
		e.dry_ref[c].resize(need); e.dry_slot[c].resize(need);
		for (int k = 0; k < need; k++) e.dry_ref[c][k] = e.dry_slot[c][k] = dry_mix(77 + c, k);
	}
	int r = TMX_OK;
	for (int n = 0; n < steps && !r; n++) {
		Program p;
		if ((r = build_program(scheme, n == 0, 0, 1.0, p, 0.0))) break;
		e.dry_copies = e.dry_shared = 0;
		r = run_program(&e, p, share == 2);      // (2: negative control of the symbolic check, every share accepted)
		// between steps instance 0 is what everything outside looks at: it must sit in its own slot and hold the reference's value
		for (int c = 0; c < 2; c++)
			if (dry_slot_of(&e, 0, c) != 0 || e.dry_slot[c][0] != e.dry_ref[c][0]) e.dry_mismatch++;
	}
	if (r) return r;
	*copies = e.dry_copies; *shared = e.dry_shared;
	return e.dry_mismatch ? -1000 - e.dry_mismatch : TMX_OK;
}

// ---------------------------------------------------------------------------------------------
// Stepper programs on the node-unique layout (UniqueLayout, tmx_internal.h; kernels instantiated with UQ = true).  The same
// programs, interpreted with the same fusion rules: [Copy | LinearCombine]; H; V; DSS is one stage (explicit kernels writing
// averaged nodes and partial slots, exchange of the slots other ranks need, k_dss_u), Copy; V.StepImplicit a U,V slab copy
// plus the column solve on the unique columns, StepAfterSubCycle its one or two passes with their DSS.  An explicit update
// that is not followed by the DSS of its instance has no node-unique form (the copies of a seam node then differ), so a program
// is run this way only if every operation fits (program_fits_unique); otherwise, and for instances whose copies differ on entry
// (a freshly uploaded initial state), tmx_step runs the element-major program.

// where a kernel that reads instance ix while producing it must write: the spare slot; u_adopt_spare makes it the instance's afterwards
static double * uspare(tmx_engine * e) { return e->u.d_ustate + (size_t)e->u.uspare * e->u.ustride; }
static void u_adopt_spare(tmx_engine * e, int ix) { std::swap(e->u.uslot[ix], e->u.uspare); }

// The node-unique interpreter's side conditions.  A stage exists only with its DSS; an explicit update without it (a bare H or V)
// has no node-unique form.
static bool unique_stage(const Unit & u) {
	return u.kind == U_STAGE && u.dss_follows && u.same_coef && u.init != u.upd && (!u.from_copy || u.base != u.upd);
}
// the operations the interpreter consumes at p[i] (a Copy in front of a column solve counts on its own here); 0: not representable
static int unique_ops(const Program & p, size_t i, const Unit & u) {
	if (unique_stage(u)) return u.n_ops + 1;
	return (p[i].kind == OP_HEXP || p[i].kind == OP_VEXP) ? 0 : 1;
}
// the number of such steps the program takes; 0: some operation has no node-unique form
static int unique_units(const Program & p) {
	int units = 0;
	for (size_t i = 0; i < p.size(); units++) { const int k = unique_ops(p, i, match_unit(p, i)); if (!k) return 0; i += k; }
	return units;
}
static bool program_fits_unique(const Program & p) { return unique_units(p) != 0; }

// Host logic for the CPU tests: does the program of a scheme have a node-unique form, and in how many units does the interpreter run it?
// Returns the number of units (fused groups of operations), 0 if some operation has no node-unique form, -1 for an unknown scheme.
extern "C" int tmx_debug_program_unique(int scheme, int first_step, int last_step) {
	Program p;
	if (build_program(scheme, first_step, last_step, 1.0, p, 0.0)) return -1;
	return unique_units(p);
}

// (the partial slots were filled by block kernels: the shorter list -- what no workgroup averaged)
static int u_dss_finish(tmx_engine * e, int ix, bool overlapped) {
	ProfScope ps(e, TMX_K_DSS);
	const UniqueLayout & u = e->u;
	const bool bl = u.slots_by_blocks;
	const int ng = bl ? u.b_ngroups : u.ngroups, nl = bl ? u.b_ngroups_local : u.ngroups_local;
	if (e->cfg.n_ranks > 1 && nl < ng) {
		tmxuk_dss(e, uinst(e, ix), 0, nl, bl);
		if (overlapped) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_recv, 0));
		tmxuk_dss(e, uinst(e, ix), nl, ng, bl);
	} else tmxuk_dss(e, uinst(e, ix), 0, ng, bl);
	return launch_check("DSS of the partial slots");
}

// kernels(KParams): the launches that fill instance ix and its partial slots; run boundary tiles first where the rank has both kinds
template <class F> static int u_produce_and_average(tmx_engine * e, int ix, int prof_slot, F kernels) {
	const UniqueLayout & u = e->u;
	KParams p = tmxu_params(e, make_params(e));
	bool overlapped = false;
	int r;
	if (u.split) {
		for (int part = 0; part < 2; part++) {
			p.quads = part ? u.d_quads_late : u.d_quads_early;
			e->launch_tiles = part ? u.n_late : u.n_early;
			p.bquads = part ? u.d_blks_late : u.d_blks_early;      // (block kernels: the same split by blocks)
			e->launch_blocks = part ? u.nb_late : u.nb_early;
			{ ProfScope ps(e, prof_slot); kernels(p); }
			if (part == 0) { p.quads = nullptr; p.bquads = nullptr; if ((r = exchange(e, p, nullptr, &overlapped))) return r; }
		}
		p.quads = nullptr; p.bquads = nullptr;
	} else {
		{ ProfScope ps(e, prof_slot); kernels(p); }
		if ((r = exchange(e, p, nullptr, &overlapped))) return r;
	}
	if ((r = launch_check("kernels of a stage (node-unique layout)"))) return r;
	return u_dss_finish(e, ix, overlapped);
}

// A stage "LinearCombine(lc -> d); H; V; DSS(d)" at operation i whose sources are exactly the LEADING terms of a later such
// stage's combination (in the reference's accumulation order: the destination's own term, then ascending instance index), none of
// them written in between: it also stores that leading partial sum (EmitTerms), and the later stage starts from it.
// ARS343 (the bench): stage 3 reads instances 0..4, stage 4 combines 1, 0, 2, 3, 4, 5, 6 -- it reads the prefix, 5 and 6.
struct PrefixPlan {
	size_t producer = 0, consumer = 0;      // operation index of the two stages' LinearCombine
	unsigned members = 0u;    // instances the prefix holds
	int first = -1;           // producer's term index of the consumer's destination (-1: the consumer's own coefficient is zero)
	double coef[12];          // consumer's coefficient of the producer's term m
};
static bool lincomb_stage(const Unit & u) { return u.lc && unique_stage(u); }
static bool prefix_plan(const tmx_engine * e, const Program & p, size_t i, Access ax, PrefixPlan * plan) {
	const Op & R = p[i];
	const Unit u = match_unit(p, i);
	if (!e->u.prefix_option || !lincomb_stage(u) || R.lc[R.a] != 0.0) return false;
	int term_of[32]; unsigned A = 0u; int nA = 0;
	for (int m = 0; m < 32; m++) term_of[m] = -1;
	for (int m = 0; m < R.nlc && m < 32; m++) if (m != R.a && R.lc[m] != 0.0) { term_of[m] = 1 + nA++; A |= 1u << m; }
	if (nA < 2 || nA > 7) return false;      // (the kernels that store a prefix: 3 to 8 terms, the destination's unread one included)
	for (size_t j = i + u.n_ops + 1; j < p.size(); j++) {
		const Op & S = p[j];
		if (S.kind == OP_LINCOMB && lincomb_stage(match_unit(p, j))) {
			unsigned B = 0u;
			for (int m = 0; m < S.nlc && m < 32; m++) if (S.lc[m] != 0.0) B |= 1u << m;
			if ((B & A) == A && (B & ~A) != 0u) {
				// order: [S.a if its coefficient is not zero], then ascending -- the members first
				int top = -1, low = 32;      // last member and first other term of the ascending part
				for (int q = 0; q < 32; q++) if ((A >> q & 1u) && q != S.a) top = q;
				for (int q = 31; q >= 0; q--) if ((B & ~A) >> q & 1u) low = q;
				if ((!(B >> S.a & 1u) || (A >> S.a & 1u)) && low > top) {
					plan->producer = i; plan->consumer = j; plan->members = A; plan->first = (A >> S.a & 1u) ? term_of[S.a] : -1;
					for (int m = 0; m < 12; m++) plan->coef[m] = 0.0;
					for (int m = 0; m < 32; m++) if (term_of[m] >= 0) plan->coef[term_of[m]] = S.lc[m];
					return true;
				}
			}
		}
		const OpAccess x = op_access(S, ax);
		if ((x.full | x.part) & A) return false;      // a member is rewritten: no later stage sees these values
	}
	return false;
}

// the producer / consumer pairs of a program that are used: there is one prefix slot, so their spans must not touch; the pairs that
// save the most source instances first (ARS343: the third stage's five sources serve the fourth -- four instances less to read --
// rather than the second stage's three serving the third)
static std::vector<PrefixPlan> prefix_schedule(const tmx_engine * e, const Program & p, Access ax) {
	std::vector<PrefixPlan> all, use;
	for (size_t i = 0; i < p.size(); ) {
		const int k = unique_ops(p, i, match_unit(p, i));
		if (!k) return use;
		PrefixPlan plan;
		if (prefix_plan(e, p, i, ax, &plan)) all.push_back(plan);
		i += k;
	}
	auto saved = [](const PrefixPlan & a) { int c = 0; for (int m = 0; m < 32; m++) c += a.members >> m & 1u; return c - 1; };
	std::stable_sort(all.begin(), all.end(), [&](const PrefixPlan & a, const PrefixPlan & b) { return saved(a) > saved(b); });
	for (const PrefixPlan & a : all) {
		bool clash = false;
		for (const PrefixPlan & b : use) clash = clash || !(a.consumer < b.producer || b.consumer < a.producer);
		if (!clash) use.push_back(a);
	}
	std::sort(use.begin(), use.end(), [](const PrefixPlan & a, const PrefixPlan & b) { return a.producer < b.producer; });
	return use;
}

extern "C" int tmx_debug_program_prefix(int scheme, int first_step, int last_step, int * pairs, int * terms, int cap) {
	Program p;
	if (build_program(scheme, first_step, last_step, 1.0, p, 0.0)) return -1;
	tmx_engine e;      // (only the option is read)
	e.u.prefix_option = 1;
	if (!program_fits_unique(p)) return 0;
	const Access ax = { false, true, false };
	const std::vector<PrefixPlan> use = prefix_schedule(&e, p, ax);
	int n = 0;
	for (const PrefixPlan & plan : use) {
		if (n < cap) {
			if (pairs) { pairs[2 * n] = (int)plan.producer; pairs[2 * n + 1] = (int)plan.consumer; }
			if (terms) { int c = 0; for (int m = 0; m < 32; m++) c += plan.members >> m & 1u; terms[n] = c - 1; }
		}
		n++;
	}
	return n;
}

// [Copy(ibase -> iupd) | LinearCombine(lc -> iupd)]; H.StepExplicit(iinit, iupd); V.StepExplicit(iinit, iupd); DSS(iupd)
// emit: also store the prefix of a later stage's combination; held: members of the stored prefix this stage's combination starts from
static int u_stage(tmx_engine * e, int iinit, int ibase, int iupd, double dt, const double * lc, int nlc, const PrefixPlan * emit = nullptr, unsigned held = 0u) {
	double * const prefix = e->u.d_ustate + (size_t)e->u.uprefix * e->u.ustride;
	// instances read in element-major form, copy by copy (UniqueLayout::dlive): their pointers are the element-major slots', the kernels get a mask
	const WhereU where = { e, e->u.dlive };
	// (all pointers are taken here, before the update instance changes slots)
	StageIO st; st.dt = dt; st.fuse_v = 1; st.emit = nullptr;
	StageTerms & t = st.base;
	if (lc) {
		REQUIRE(gather_terms(t, lc, nlc, iupd, held, where), TMX_ERR_UNSUPPORTED, "linear combination with more than 11 source terms");
		if (held) { t.src[0] = t.src_uv[0] = prefix; t.coef[0] = 1.0; t.premul = 1; e->u.prefix_stages++; }      // (times one: exact)
	} else t = base_terms(ibase, where);
	if (where(iinit, st.xin, st.xin_uv)) t.dmask |= 1u << 31;
	const int n = t.n; const unsigned dmask = t.dmask;
	REQUIRE(!(held && dmask), TMX_ERR_UNSUPPORTED, "internal: stored prefix with element-major sources");
	REQUIRE(!dmask || e->u.tile_shape == 0 || tmxk_h_walk_ok(e, tmxu_params(e, make_params(e)), 1, n, false), TMX_ERR_UNSUPPORTED,
		"internal: copy-by-copy reads of an element-major instance with this thread order need the column-segment walk");
	// the update instance is also read (in-place accumulation, or its own coefficient in the combination is not zero): the
	// element-major kernels read and write a thread's own column, here other elements' threads read the node too -- write the
	// spare slot and let it become the instance's
	bool aliased = lc ? (t.premul != 0) : (ibase == iupd);
	if (held) {      // the destination's own term is inside the prefix: its slot is read only if something else lives there
		const double * mine = uinst(e, iupd);
		aliased = st.xin_uv == mine;
		for (int m = 1; m < n; m++) aliased = aliased || t.src[m] == mine || t.src_uv[m] == mine;
	}
	REQUIRE(iinit != iupd, TMX_ERR_INVALID, "StepExplicit: initial and update data instance must be distinct");
	st.xup = aliased ? uspare(e) : uinst(e, iupd);
	EmitTerms em; em.xp = nullptr; em.first = -1;
	// (only a kernel that really stores it: the column-segment walk, or the level-parallel kernel of the experiments flavour; element-major sources: no prefix)
	const bool walk = tmxk_h_walk_ok(e, tmxu_params(e, make_params(e)), 1, n, true);
	if (emit && lc && !t.premul && n >= 3 && n <= 8 && !dmask && (walk ? !tmxu_blocks_on(e, 1) : TMX_EXP != 0)) {      // (the block form of the walk stores none)
		em.xp = prefix; em.first = emit->first; for (int m = 0; m < 12; m++) em.coef[m] = emit->coef[m];
		st.emit = &em;
	}
	if (emit) e->u.prefix_for = em.xp ? (long long)emit->consumer : -1;      // which operation may start from the stored prefix (run_program_unique)
	// the stage writes every slab of the update instance: its U,V slabs are its own from here on (what it shared is read through
	// the pointers taken above), and whoever shared ITS slabs is dead
	if (e->uvmap[iupd] != iupd) { e->uvmap[iupd] = iupd; e->n_uvshared--; }
	if (aliased) u_adopt_spare(e, iupd);      // (the stage's pointers were taken before: they still name the old slots)
	int r = u_produce_and_average(e, iupd, TMX_K_H_EXPLICIT, [&](const KParams & p) { tmxk_h_explicit(e, p, st); });
	e->u.dlive &= ~(1u << iupd);      // the instance is node-unique from here on
	u_written(e, iupd);
	if (r) return r;
	return lc ? surface_lincomb(e, lc, nlc, iupd) : surface_copy(e, ibase, iupd);      // (all terms: no prefix there)
}

static int u_copy(tmx_engine * e, int a, int b, size_t doubles) {
	if (a == b) return TMX_OK;
	int r;
	if ((r = u_own_uv(e, a)) || (r = u_own_uv(e, b, true))) return r;
	{
		ProfScope ps(e, TMX_K_LINCOMB);
		HIPCHK(hipMemcpyAsync(uinst(e, b), uinst(e, a), doubles * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
	}
	if (doubles == e->u.ustride) e->u.dlive &= ~(1u << b);
	u_written(e, b);
	return surface_copy(e, a, b);
}

// [Copy(a -> b);] V.StepImplicit(b, b): the solve rewrites rho*theta, W, rho of every column, so only the U,V slabs are copied
// share: b's U,V slabs are not copied, b reads a's (decided on the program by share_is_safe, as in the element-major interpreter)
static int u_vimp(tmx_engine * e, int a, int b, double dt, bool share) {
	REQUIRE(dt != 0.0, TMX_ERR_INVALID, "StepImplicit: dt must be non-zero");
	int r;
	if ((r = u_own_uv(e, a))) return r;      // the column kernel reads U,V of the initial instance through its one pointer
	if (a != b) {
		if (share) {
			if ((r = u_own_uv(e, b, true)) || (r = surface_copy(e, a, b))) return r;
		} else if ((r = u_copy(e, a, b, (size_t)2 * e->L * e->u.NUS))) return r;
	}
	{
		ProfScope ps(e, TMX_K_VI_SOLVE);
		e->vi_unique = true;
		tmxk_vi_fused(e, tmxu_params_columns(e, make_params(e)), uinst(e, a), uinst(e, b), dt);
		e->vi_unique = false;
	}
	e->u.dlive &= ~(1u << b);      // b is node-unique in every slab from here on (its U,V copied or shared from a, the rest solved): a later stage must not read a stale element-major slot
	u_written(e, b);
	if (a != b && share) { e->uvmap[b] = a; e->n_uvshared++; }
	return launch_check("column solve (node-unique layout)");
}

// VerticalDynamicsFEM::StepImplicitTermsExplicitly (ARK232): update -= dt F(initial) for rho*theta, W, rho, column by column -- on the
// unique columns (every copy of a node would receive the same increment of the same value)
static int u_vite(tmx_engine * e, int a, int b, double dt) {
	REQUIRE(a != b && dt != 0.0, TMX_ERR_INVALID, "StepImplicitTermsExplicitly: distinct instances and non-zero dt required");
	int r;
	if ((r = u_own_uv(e, a))) return r;      // (the kernel reads U,V of the initial instance through its one pointer)
	{
		ProfScope ps(e, TMX_K_VI_ASSEMBLE);
		tmxk_vi_terms_explicit(e, tmxu_params_columns(e, make_params(e)), uinst(e, a), uinst(e, b), dt, false);
	}
	u_written(e, b);
	return launch_check("explicitly evaluated implicit terms (node-unique layout)");
}

// DSS of an instance whose copies already agree inside every patch (e.g. after the column solve): only the nodes on patch edges change
static int u_dss(tmx_engine * e, int ix) {
	bool overlapped = false;
	int r;
	if ((r = u_own_uv(e, ix))) return r;
	{ ProfScope ps(e, TMX_K_DSS); tmxuk_slots_from_u(e, uinst(e, ix)); }
	e->u.slots_by_blocks = tmxu_blocks_on(e);      // every slot holds its node's value: the shorter list changes the same nodes (a group of identical copies averages to itself)
	if ((r = exchange(e, tmxu_params(e, make_params(e)), nullptr, &overlapped))) return r;
	r = u_dss_finish(e, ix, overlapped);
	u_written(e, ix);
	return r;
}

// HorizontalDynamicsFEM::StepAfterSubCycle (h_step_after_subcycle_impl above, same branches)
static int u_hvis_core(tmx_engine * e, int iinit, int iupd, int iwork, double dt);
// ... and its Rayleigh friction (APPLY_RAYLEIGH_WITH_HYPERVIS, HorizontalDynamicsFEM.cpp:2719-2724, ApplyRayleighFriction :2420-2570): the
// reference relaxes every stored copy with the copy's own strength and reference state, so the result has no node-unique form -- the kernel
// reads the node-unique instance and writes the element-major one, and the next step's explicit stages read that copy by copy ("unique_mixed")
static int u_hvis(tmx_engine * e, int iinit, int iupd, int iwork, double dt) {
	int r = u_hvis_core(e, iinit, iupd, iwork, dt);
	if (r || !e->rayleigh) return r;
	UniqueLayout & u = e->u;
	REQUIRE(e->imap[iupd] == iupd, TMX_ERR_INVALID, "internal: Rayleigh friction on a shared slot");
	if ((r = u_own_uv(e, iupd))) return r;
	{
		ProfScope ps(e, TMX_K_HYPERVIS);
		tmxk_rayleigh(e, make_params(e), inst(e, iupd), dt, uinst(e, iupd), (size_t)u.NUS, (const int *)u.d_ucol_of_dcol);
	}
	if (u.form[iupd]) { u.form[iupd] = 0; u.n_uform--; }
	u.conversions++;
	return launch_check("rayleigh friction (node-unique in, element-major out)");
}
static int u_hvis_core(tmx_engine * e, int iinit, int iupd, int iwork, double dt) {
	const tmx_config & c = e->cfg;
	int r;
	REQUIRE(iinit != iwork && iupd != iwork && iinit != iupd, TMX_ERR_UNSUPPORTED, "StepAfterSubCycle on the node-unique layout needs three distinct instances");
	if (!hypervis_active(e)) return u_copy(e, iinit, iupd, e->u.ustride);
	// the passes read their source through one pointer and rewrite update and (two passes) working instance entirely
	if ((r = u_own_uv(e, iinit)) || (r = u_own_uv(e, iupd, true))) return r;
	if (c.hypervis_order != 2 && (r = u_own_uv(e, iwork, true))) return r;
	struct Written { tmx_engine * e; int a, b; ~Written() { e->u.dlive &= ~(1u << a); u_written(e, a); if (b >= 0) { e->u.dlive &= ~(1u << b); u_written(e, b); } } } written = { e, iupd, c.hypervis_order != 2 ? iwork : -1 };
	if (c.hypervis_order == 2) {
		if ((r = surface_copy(e, iinit, iupd))) return r;
		return u_produce_and_average(e, iupd, TMX_K_HYPERVIS, [&](const KParams & p) {
			tmxk_hypervis(e, p, uinst(e, iinit), uinst(e, iinit), uinst(e, iupd), -dt, -c.nu_scalar, c.nu_div, c.nu_vort, 0); });
	}
	if ((r = surface_copy(e, iinit, iupd)) || (r = surface_zero(e, iwork))) return r;
	if ((r = u_produce_and_average(e, iwork, TMX_K_HYPERVIS, [&](const KParams & p) { hvis_laplacians(e, p, uinst(e, iinit), uinst(e, iwork)); }))) return r;
	return u_produce_and_average(e, iupd, TMX_K_HYPERVIS, [&](const KParams & p) { hvis_apply(e, p, uinst(e, iwork), uinst(e, iinit), uinst(e, iupd), dt); });      // (no tracers on this layout)
}

static int run_program_unique(tmx_engine * e, const Program & p, Access ax) {
	int r;
	const std::vector<PrefixPlan> plans = prefix_schedule(e, p, ax);
	e->u.prefix_for = -1;
	auto plan_at = [&](size_t i, bool consumer) -> const PrefixPlan * {
		for (const PrefixPlan & a : plans) if ((consumer ? a.consumer : a.producer) == i) return &a;
		return nullptr;
	};
	// U,V slabs still shared from the previous step: kept where this program allows it
	for (int b = 0; b < (int)e->uvmap.size() && e->n_uvshared; b++)
		if (e->uvmap[b] != b && !share_is_safe(p, 0, e->uvmap[b], b, ax) && (r = u_own_uv(e, b))) return r;
	for (size_t i = 0, ops = 0; i < p.size(); i += ops) {
		const Op & o = p[i];
		const Unit u = match_unit(p, i);
		ops = unique_ops(p, i, u);
		REQUIRE(ops, TMX_ERR_UNSUPPORTED, "internal: operation %d has no node-unique form", o.kind);
		if (unique_stage(u)) {
			const PrefixPlan * held = plan_at(i, true);      // an earlier stage has stored the leading partial sum of this combination ...
			if (held && e->u.prefix_for != (long long)i) held = nullptr;      // ... unless it could not (it read an element-major instance copy by copy)
			if ((r = u_stage(e, u.init, u.base, u.upd, u.coef, u.lc, u.nlc, plan_at(i, false), held ? held->members : 0u))) return r;
			continue;
		}
		if (u.kind == U_COPY_VIMP) {      // Copy(s -> t) [repeated] + V.StepImplicit(t, t)
			const bool share = e->share_copies && e->uvmap[u.base] == u.base && share_is_safe(p, i + u.n_ops, u.base, u.upd, ax);
			if ((r = u_vimp(e, u.base, u.upd, u.coef, share))) return r;
			ops = u.n_ops;
			continue;
		}
		switch (o.kind) {
		case OP_COPY:
			if (u.kind == U_COPY_HVIS) break;      // Copy(a -> b) + StepAfterSubCycle(a, b, w): every branch rewrites all of b from a
			if (!e->u.form[o.a] && o.a != o.b) {
				// the source is element-major: the Rayleigh relaxation at the end of StepAfterSubCycle left it so (u_hvis); the copy is
				// a whole-slot copy as in the element-major program (surface slots included), and the destination is element-major too
				REQUIRE(e->rayleigh && e->imap[o.a] == o.a && e->imap[o.b] == o.b, TMX_ERR_INVALID, "internal: element-major source of a copy inside a node-unique program");
				if ((r = u_own_uv(e, o.b, true))) return r;
				{
					ProfScope ps(e, TMX_K_LINCOMB);
					HIPCHK(hipMemcpyAsync(inst(e, o.b), inst(e, o.a), e->inst_stride * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
				}
				if (e->u.form[o.b]) { e->u.form[o.b] = 0; e->u.n_uform--; }
				e->u.dlive &= ~(1u << o.b);
				u_written(e, o.b);
				break;
			}
			if ((r = u_copy(e, o.a, o.b, e->u.ustride))) return r;
			break;
		case OP_LINCOMB: {
			if ((r = u_own_uv(e, o.a, o.lc[o.a] == 0.0))) return r;
			for (int m = 0; m < o.nlc; m++) if (m != o.a && o.lc[m] != 0.0 && (r = u_own_uv(e, m))) return r;      // (whole-instance pass: one pointer per source)
			StageTerms t;
			REQUIRE(gather_terms(t, o.lc, o.nlc, o.a, 0u, WhereU{ e, 0u }), TMX_ERR_UNSUPPORTED, "linear_combine_data: more than 11 source terms");
			{ ProfScope ps(e, TMX_K_LINCOMB); tmxk_lincomb(e, e->u.ustride, uinst(e, o.a), t); }
			e->u.dlive &= ~(1u << o.a);
			u_written(e, o.a);
			if ((r = surface_lincomb(e, o.lc, o.nlc, o.a)) || (r = launch_check("lincomb"))) return r;
			break; }
		case OP_VIMP: if ((r = u_vimp(e, o.a, o.b, o.coef, false))) return r; break;
		case OP_DSS: if ((r = u_dss(e, o.a))) return r; break;
		case OP_HVIS: if ((r = u_hvis(e, o.a, o.b, o.c, o.coef))) return r; break;
		case OP_VITE: if ((r = u_vite(e, o.a, o.b, o.coef))) return r; break;
		case OP_VFILT: break;      // nothing without tracers
		}
	}
	return TMX_OK;
}

// May the program read the instances of `dlive` in element-major form, copy by copy?  Only the explicit stages can (their kernels take a
// source mask); every other operation must find the instance overwritten -- node-unique -- by the time it reads it.
static bool dlive_program_ok(const Program & p, unsigned dlive, Access ax) {
	for (size_t i = 0; i < p.size() && dlive; ) {
		const Unit u = match_unit(p, i);
		const int k = unique_ops(p, i, u);
		if (!k) return false;
		unsigned wr = 0u;
		for (int j = 0; j < k; j++) {
			const OpAccess x = op_access(p[i + j], ax);
			if (!unique_stage(u) && ((x.reads | x.part) & dlive)) return false;
			wr |= x.full | x.part;
		}
		dlive &= ~wr;
		i += k;
	}
	return true;
}
// Host logic for the CPU tests: can the scheme's program read instance `instance` copy by copy (1), or not (0)?  -1: unknown scheme
extern "C" int tmx_debug_program_mixed(int scheme, int first_step, int last_step, int instance) {
	Program p;
	if (build_program(scheme, first_step, last_step, 1.0, p, 0.0)) return -1;
	const Access ax = { false, true, false };
	return (program_fits_unique(p) && dlive_program_ok(p, 1u << instance, ax)) ? 1 : 0;
}

// Entry of tmx_step: bring the instances the program reads before it overwrites them into the node-unique form (checking, for
// those that come from the element-major form, that the copies of every node agree) and run the program there.  *done = false:
// not possible (configuration, program, or an instance whose copies differ); the caller runs the element-major program.
// With a Rayleigh layer the result of StepAfterSubCycle is element-major (u_hvis): the node-unique interpreter serves the programs in which
// only copies of that result follow (ARS343: nothing follows; ARS222 / 232 / 443 / ARK232: Copy(result -> 0)); Strang's closing column solve
// of the relaxed state has no node-unique form, its programs stay element-major
static bool rayleigh_program_ok(const Program & p) {
	size_t h = p.size();
	for (size_t i = 0; i < p.size(); i++) if (p[i].kind == OP_HVIS) { if (h != p.size()) return false; h = i; }
	for (size_t i = h + 1; i < p.size(); i++) if (!(p[i].kind == OP_COPY && p[i].a == p[h].b)) return false;
	return true;
}
// Host logic for the CPU tests: with a Rayleigh layer, does the scheme's program run on the node-unique layout (1) or element-major (0)?  -1: unknown scheme
extern "C" int tmx_debug_program_rayleigh(int scheme, int first_step, int last_step) {
	Program p;
	if (build_program(scheme, first_step, last_step, 1.0, p, 0.0)) return -1;
	return (program_fits_unique(p) && rayleigh_program_ok(p)) ? 1 : 0;
}
static int try_step_unique(tmx_engine * e, const Program & p, bool * done) {
	*done = false;
	UniqueLayout & u = e->u;
	if (!u.built || !program_fits_unique(p)) return TMX_OK;
	if (e->rayleigh && !rayleigh_program_ok(p)) return TMX_OK;
	// StepImplicitTermsExplicitly evaluates EVERY stored copy of a node with the copy's own column metric (VerticalDynamicsFEM.cpp:543-566:
	// all interior (i, j), none skipped); the node-unique form evaluates the representative copy once, which is the same only where the
	// copies' metric entries carry the same bits (UniqueLayout::vite_ok, checked on the host's arrays when the layout is built)
	if (!u.vite_ok) for (const Op & o : p) if (o.kind == OP_VITE) return TMX_OK;
	int r;
	unsigned written = 0u, livein = 0u;
	const Access ax = { false, hypervis_active(e) && e->cfg.hypervis_order != 2, false };
	for (size_t i = 0; i < p.size(); i++) {
		const OpAccess x = op_access(p[i], ax);
		livein |= x.reads & ~written;
		livein |= x.part & ~written;
		written |= x.full | x.part;
	}
	bool need_check = false;
	unsigned dform = 0u;
	for (int k = 0; k < e->cfg.n_instances; k++) if ((livein >> k & 1u) && !u.form[k]) { need_check = true; dform |= 1u << k; }
	// Round 5: live-in instances in element-major form are READ that way, copy by copy, by the explicit stages (no check of the copies, no
	// host synchronisation, no conversion; exact whether the copies agree or not) wherever the program lets only its stages read them
	u.dlive = 0u;
	// (a thread reads its own stored copy: the level-parallel kernels take the thread index for the stored column, which only the default thread order
	// allows; the column-segment walk looks the column up, KParams::t_dcol)
	const bool own_copy_ok = u.tile_shape == 0 || (u.tile_shape == 4 && e->opt_h_walk != 0 && !e->use_mfma);
	if (dform && u.mixed_option && own_copy_ok && dlive_program_ok(p, dform, ax)) {
		for (int k = 0; k < e->cfg.n_instances; k++)
			if ((dform >> k & 1u) && (e->imap[k] != k || e->uvmap[k] != k) && (r = settle_instance(e, k, false))) return r;
		u.dlive = dform; need_check = false; u.mixed_steps++;
	}
	if (need_check && u.skip_steps > 0) { u.skip_steps--; return TMX_OK; }      // the last checks failed: not every step pays for another one
	// (timing aid TMX_DEBUG_SKIP_EXCHANGE: the state of such a run is garbage at the rank boundary, NaN payloads included; no check)
	const bool trust = TMX_EXP && e->opt_skip_exchange != 0;
	// the check comes first and works on the slots as the element-major programs left them (shared slots included: an instance
	// that shares is given its own first, which for the model state never happens), so that a step that stays element-major keeps them
	for (int k = 0; k < e->cfg.n_instances && !trust && !u.dlive; k++) {
		if (!(livein >> k & 1u) || u.form[k]) continue;
		if ((e->imap[k] != k || e->uvmap[k] != k) && (r = settle_instance(e, k, false))) return r;
		bool ok = true;
		if ((r = tmxu_check(e, k, &ok))) return r;
		if (!ok) {      // copies differ: this step runs element-major
			// (a single failure -- the pointwise initial state of a run -- costs nothing further; from the second in a row on, 4, 8, ... 1024 steps pass before the next try)
			u.backoff++;
			u.skip_steps = (u.backoff >= 2) ? std::min(4 << std::min(u.backoff - 2, 8), 1024) : 0;
			return TMX_OK;
		}
	}
	u.backoff = 0;
	// instance maps to identity (shares left by an element-major program, that is: nothing is in U form; U,V slabs shared by the last node-unique step stay shared)
	if ((e->n_shared || e->n_uvshared) && u.n_uform == 0) { if ((r = settle_instance(e, -1, false))) return r; }
	for (int k = 0; k < e->cfg.n_instances; k++)
		if ((livein >> k & 1u) && !u.form[k] && !(u.dlive >> k & 1u) && (r = tmxu_to_u(e, k, false, nullptr))) return r;
	// everything the program writes is in U form afterwards; whatever else it leaves alone keeps its form
	for (int k = 0; k < e->cfg.n_instances; k++)
		if (written >> k & 1u) { if (!u.form[k]) u.n_uform++; u.form[k] = 1; }      // (form 2 -> 1: the element-major copy goes stale)
	e->in_program = true;
	r = run_program_unique(e, p, ax);
	e->in_program = false;
	u.dlive = 0u;
	*done = true;
	return r;
}

extern "C" int tmx_scheme_instances(int scheme) { return scheme_instances(scheme); }

extern "C" int tmx_step(tmx_engine * e, int scheme, int first_step, int last_step, double dt) {
	int r; if ((r = check_ready(e))) return r;
	const int need = scheme_instances(scheme);
	REQUIRE(need > 0, TMX_ERR_INVALID, "unknown time scheme %d", scheme);
	REQUIRE(e->cfg.n_instances >= need, TMX_ERR_INVALID, "time scheme %d needs %d data instances, engine has %d", scheme, need, e->cfg.n_instances);
	if ((r = tmx_vertical_fit(e, tmx_vertical_fit_of_step(e)))) return r;      // a level count a vertical launcher of this configuration does not serve: refused before the step's first kernel
	Program p;
	if ((r = build_program(scheme, first_step, last_step, dt, p, e->strang_offc))) return r;
	// Optional (TMX_GRAPH=1): single-rank steps replayed from a hipGraph -- the 20-30 launches of a step are
	// captured once per (scheme, first, last, dt), every kernel argument being fixed after tmx_finalize, and
	// relaunched as one graph.  Off by default: the plain sequence is already queued asynchronously far ahead of the
	// GPU, and the replay measured 0-1 % SLOWER (ne8: 0.419 vs 0.414 ms/step, ne16: 0.605 vs 0.601, ne30: 1.65 both).
	// Multi-rank steps (RCCL calls on a second stream) and profiled steps always use the plain sequence.
	if (e->use_graph && (e->cfg.n_ranks == 1 || (TMX_EXP && e->opt_skip_exchange)) && !e->prof && !e->lb) {
		StepGraphKey key = { scheme, first_step ? 1 : 0, last_step ? 1 : 0, dt };
		if (e->udiff) {      // (the reference state's stored diffusion terms: allocated and formed outside the capture)
			bool all = true;
			for (int lp : e->local_patches) all = all && e->patches[lp].ref_set;
			if (all) tmxk_h_walk_prepare(e, make_params(e));
		}
		for (auto & g : e->graphs)
			if (g.key.scheme == key.scheme && g.key.first == key.first && g.key.last == key.last && g.key.dt == key.dt) {
				HIPCHK(hipGraphLaunch(g.exec, e->stream));
				return TMX_OK;
			}
		hipGraph_t graph = nullptr;
		HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
		r = run_program(e, p);
		const hipError_t ce = hipStreamEndCapture(e->stream, &graph);
		if (r) { if (graph) hipGraphDestroy(graph); (void)hipGetLastError(); return r; }      // (the error is reported; it must not stay behind as the runtime's last error)
		if (ce != hipSuccess || !graph) {
			(void)hipGetLastError();
			e->use_graph = false;                 // capture not possible here: run the plain sequence from now on
			return run_program(e, p);
		}
		StepGraph sg; sg.key = key;
		const hipError_t ie = hipGraphInstantiate(&sg.exec, graph, nullptr, nullptr, 0);
		hipGraphDestroy(graph);
		if (ie != hipSuccess) { (void)hipGetLastError(); e->use_graph = false; return run_program(e, p); }
		if (e->graphs.size() >= 8) { hipGraphExecDestroy(e->graphs.front().exec); e->graphs.erase(e->graphs.begin()); }
		e->graphs.push_back(sg);
		HIPCHK(hipGraphLaunch(sg.exec, e->stream));
		return TMX_OK;
	}
	if (e->u.built) {
		bool done = false;
		if ((r = try_step_unique(e, p, &done)) || done) return r;
		// element-major step: nothing stays in U form (the shared slots of the element-major programs are left as they are)
		if (e->u.n_uform)
			for (int b = 0; b < (int)e->u.form.size(); b++) if (e->u.form[b] && (r = tmxu_to_d(e, b))) return r;
	}
	return run_program(e, p);
}

extern "C" int tmx_set_strang_off_centering(tmx_engine * e, double off_centering) {
	REQUIRE(e, TMX_ERR_INVALID, "tmx_set_strang_off_centering: null engine");
	REQUIRE(off_centering >= 0.0 && off_centering <= 1.0, TMX_ERR_INVALID, "off-centering %g outside [0, 1] (TimestepSchemeStrang.cpp:34-36)", off_centering);
	if (off_centering != e->strang_offc) {
		if (!plan_only(e) && e->stream) hipStreamSynchronize(e->stream);
		for (auto & g : e->graphs) hipGraphExecDestroy(g.exec);      // captured steps carry the old coefficients
		e->graphs.clear();
	}
	e->strang_offc = off_centering;
	return TMX_OK;
}

extern "C" int tmx_step_ars343(tmx_engine * e, double dt) { return tmx_step(e, TMX_SCHEME_ARS343, 0, 0, dt); }

