// tmx_device_column.h -- the block-row assembly of the vertical operator: residual F and analytic band Jacobian of one block row
// (level) of one column (VerticalDynamicsFEM::PrepareColumn / BuildF / BuildJacobianF_*), shared by the column solve (tmx_k_column.hip:
// F and the Jacobian, ahead of the band LU) and by StepImplicitTermsExplicitly (tmx_k_vertical.hip: F alone).  Nothing here uses
// LU_UPD, so it compiles to the same instructions in either rounding of the band LU.  gfx950 only.
#pragma once
#include "tmx_device.h"

// band offset of column (c', k') seen from row (c, k) of the block matrix: d = 3(k'-k) + (c'-c) + 4
#define DOFF(cr, cc_, dk) (3 * (dk) + ((cc_) - (cr)) + 4)

struct NodeLev { double un, vn, pn, rn, ca2, cb2, cx2; };
struct EdgeLev { double we, ce0, ce1, ce2; };

// Loads are unconditional with the level clamped into range: a fixed number of loads per block row keeps the
// compiler's vmcnt bookkeeping exact, so a wait for the previous block row's prefetch does not also wait for
// the loads just issued.  Out-of-range levels (-1 below block row 0, L and L+1 past the top) therefore carry
// the values of the nearest level; compute_block only touches them under its k >= 1 / k + 1 <= L - 1 guards or
// with zero operator coefficients, so results do not depend on them (checked bitwise against the split kernels).
template <int MM = 0>
__device__ __forceinline__ NodeLev load_node(const KParams & p, const MetCol & mc, const double * xin, int l, int col, const double * etal = nullptr) {
	NodeLev n;
	const int L = p.L;
	const int lc = l < 0 ? 0 : (l >= L ? L - 1 : l);
	const size_t NS = (size_t)p.NS;
	n.un = xin[TMX_SLAB_U(L, lc) * NS + col]; n.vn = xin[TMX_SLAB_V(L, lc) * NS + col];
	n.pn = xin[TMX_SLAB_T(L, lc) * NS + col]; n.rn = xin[TMX_SLAB_R(L, lc) * NS + col];
	metric_node3<MM>(p, mc, lc, col, n.ca2, n.cb2, n.cx2, etal);
	return n;
}
template <int MM = 0>
__device__ __forceinline__ EdgeLev load_edge(const KParams & p, const MetCol & mc, const double * xin, int l, int col, const double * etal = nullptr) {
	EdgeLev e;
	const int L = p.L;
	const int lc = l < 0 ? 0 : (l > L ? L : l);
	const size_t NS = (size_t)p.NS;
	e.we = xin[TMX_SLAB_W(L, lc) * NS + col];
	metric_edge<MM>(p, mc, lc, col, e.ce0, e.ce1, e.ce2, etal);
	return e;
}

struct ColConst { double c2a0, c2a1, c2b1, jn, je, drx, invdt, upc, cv; };

// Values one block row shares with the next (level k quantities become level k-1 quantities, interface
// k+1 quantities become interface k quantities).  Carrying them over instead of recomputing is the same
// arithmetic on the same operands, so results stay bit-identical to the stand-alone evaluation.
struct BlkCarry {
	double ex, wn, xdn, ke;            // node k: Exner pressure, W on the level, xi_dot, kinetic energy
	double ue, ve, xd, pe, re;         // interface k+1: U,V, xi_dot, rho*theta, rho interpolated
};

// block row k from node levels A = k-1, B = k, C = k+1 and interfaces a = k-1, b = k, c = k+1
// column-operator coefficients from the LDS copy (ds_read: no vector-memory round trip, no vmcnt wait behind the U-row stores)
// UD: the uniform-diffusion terms of BuildF (VerticalDynamicsFEM.cpp:2593-2635), udP = K_s / ztop^2 * second derivative
// of (rho*theta - reference) on level k, udW = K_v / ztop^2 * the same for W on interface k, subtracted where the
// reference subtracts them (before the upwinding terms); only the fully explicit mode evaluates them.
// sign(x) * v as in the reference's upwinding terms ((x > 0) ? v : ((x < 0) ? -v : 0)), written as a chain of two selects: the
// nested conditional became exec-masked branches, which cut the block row's assembly into short basic blocks
__device__ __forceinline__ double signed_by(double x, double v) {
	double r = 0.0;
	r = (x < 0.0) ? -v : r;
	r = (x > 0.0) ? v : r;
	return r;
}

// INTERIOR: the caller guarantees 1 <= k <= L - 2 and arguments of the Exner function in the main range of exp / log (positive,
// normal, finite): every level-boundary condition below is then a compile-time `true` and exp(log()) is evaluated without
// branches (exner_from_rhotheta_bf), so that the whole block row is ONE basic block whose dependency chains the compiler can
// interleave -- with the dozen short blocks of the general form a lone assembly wavefront ran at a quarter of its issue rate.
// Same statements on the same operands either way.
template <bool CARRY, bool UD = false, bool INTERIOR = false>
__device__ __forceinline__ void compute_block(const KParams & p, const double * opsl, const ColConst & cc, int k,
	const NodeLev & A, const NodeLev & B, const NodeLev & C, const EdgeLev & ea, const EdgeLev & eb, const EdgeLev & ec,
	double * rowP, double * rowW, double * rowR, double & fP, double & fW, double & fR, BlkCarry & cy,
	double udP = 0.0, double udW = 0.0, const double * rmtab = nullptr, long long * tseg = nullptr)
{
#ifdef TMX_PAIR_TIMING
	long long ts_ = __builtin_readcyclecounter();
#define CBSTAMP(i) do { if (tseg) { const long long t1_ = __builtin_readcyclecounter(); tseg[i] += t1_ - ts_; ts_ = t1_; } } while (0)
#else
#define CBSTAMP(i)
#endif
	const int L = p.L;
#pragma unroll
	for (int d = 0; d < TMX_BW; d++) { rowP[d] = 0.0; rowW[d] = 0.0; rowR[d] = 0.0; }
	fP = 0.0; fW = 0.0; fR = 0.0;
	// interior interpolation stencils (offsets -1, 0), verified by tmx_set_operators
	const int kib = (INTERIOR || k < L) ? k : L;
	const double ib_m = OPCL(TMX_OP_INTERP_NODE_TO_REDGE, kib, -1), ib_0 = OPCL(TMX_OP_INTERP_NODE_TO_REDGE, kib, 0);

	// ---- interface k: interpolated U,V,rho*theta,rho and xi_dot (PrepareColumn :2056-2069) ----
	double ue_b = 0.0, ve_b = 0.0, xd0 = 0.0, pe0 = 0.0, re0 = 0.0;
	if (INTERIOR || (k >= 1 && k <= L - 1)) {
		if (CARRY) { ue_b = cy.ue; ve_b = cy.ve; xd0 = cy.xd; pe0 = cy.pe; re0 = cy.re; }
		else {
			ue_b += ib_m * A.un; ue_b += ib_0 * B.un; ve_b += ib_m * A.vn; ve_b += ib_0 * B.vn;
			xd0 = eb.ce0 * ue_b + eb.ce1 * ve_b + eb.ce2 * eb.we;
			pe0 += ib_m * A.pn; pe0 += ib_0 * B.pn; re0 += ib_m * A.rn; re0 += ib_0 * B.rn;
		}
	}
	// ---- interface k+1 ----
	double ue_c = 0.0, ve_c = 0.0, xd1 = 0.0, pe1 = 0.0, re1 = 0.0;
	double ic_m = 0.0, ic_0 = 0.0;
	if (INTERIOR || k + 1 <= L - 1) {
		ic_m = OPCL(TMX_OP_INTERP_NODE_TO_REDGE, k + 1, -1); ic_0 = OPCL(TMX_OP_INTERP_NODE_TO_REDGE, k + 1, 0);
		ue_c += ic_m * B.un; ue_c += ic_0 * C.un; ve_c += ic_m * B.vn; ve_c += ic_0 * C.vn;
		xd1 = ec.ce0 * ue_c + ec.ce1 * ve_c + ec.ce2 * ec.we;
		pe1 += ic_m * B.pn; pe1 += ic_0 * C.pn; re1 += ic_m * B.rn; re1 += ic_0 * C.rn;
	}

	CBSTAMP(0);
	if (INTERIOR || k < L) {
		const double invJ = 1.0 / cc.jn;
		const double pm = A.pn, p0 = B.pn, pp = C.pn, rm = A.rn, r0 = B.rn, rp = C.rn;
		const double mf0 = (INTERIOR || k >= 1) ? cc.je * re0 * xd0 : 0.0, mf1 = (INTERIOR || k + 1 <= L - 1) ? cc.je * re1 * xd1 : 0.0;
		const double pf0 = (INTERIOR || k >= 1) ? cc.je * pe0 * xd0 : 0.0, pf1 = (INTERIOR || k + 1 <= L - 1) ? cc.je * pe1 * xd1 : 0.0;
		const double de0 = OPCL(TMX_OP_DIFF_REDGE_TO_NODE, k, 0), de1 = OPCL(TMX_OP_DIFF_REDGE_TO_NODE, k, 1);
		double dmf = 0.0; dmf += de0 * mf0; dmf += de1 * mf1;
		double dpf = 0.0; dpf += de0 * pf0; dpf += de1 * pf1;
		fR = dmf * invJ;
		fP += dpf * invJ;
		if (UD) fP -= udP;
		const double wlo = fabs(xd0), whi = fabs(xd1);
		const double pl0 = OPCL(TMX_OP_PENALTY_LEFT, k, 0), pl1 = OPCL(TMX_OP_PENALTY_LEFT, k, 1);
		const double pr0 = OPCL(TMX_OP_PENALTY_RIGHT, k, -1), pr1 = OPCL(TMX_OP_PENALTY_RIGHT, k, 0);
		{
			double a = 0.0;
			if (INTERIOR || k < L - 1) { double b = 0.0; b += pl0 * p0; b += pl1 * pp; a += b * whi; }
			if (INTERIOR || k > 0) { double b = 0.0; b += pr0 * pm; b += pr1 * p0; a += b * wlo; }
			fP -= a;
			a = 0.0;
			if (INTERIOR || k < L - 1) { double b = 0.0; b += pl0 * r0; b += pl1 * rp; a += b * whi; }
			if (INTERIOR || k > 0) { double b = 0.0; b += pr0 * rm; b += pr1 * r0; a += b * wlo; }
			fR -= a;
		}
		// conservative flux terms: m = k (interface b), m = k+1 (interface c)
		if (INTERIOR || k >= 1) {       // m = k, neither 0 nor L
			const double c = de0 * cc.je * invJ * eb.ce2;
			rowP[DOFF(0, 1, 0)] += c * pe0;
			rowR[DOFF(2, 1, 0)] += c * re0;
			const double cm = de0 * cc.je * invJ * ib_m * xd0, c0 = de0 * cc.je * invJ * ib_0 * xd0;
			rowR[DOFF(2, 2, -1)] += cm; rowP[DOFF(0, 0, -1)] += cm;
			rowR[DOFF(2, 2, 0)] += c0;  rowP[DOFF(0, 0, 0)] += c0;
		}
		if (INTERIOR || k + 1 <= L - 1) {   // m = k+1
			const double c = de1 * cc.je * invJ * ec.ce2;
			rowP[DOFF(0, 1, 1)] += c * pe1;
			rowR[DOFF(2, 1, 1)] += c * re1;
			const double cm = de1 * cc.je * invJ * ic_m * xd1, c0 = de1 * cc.je * invJ * ic_0 * xd1;
			rowR[DOFF(2, 2, 0)] += cm; rowP[DOFF(0, 0, 0)] += cm;
			rowR[DOFF(2, 2, 1)] += c0; rowP[DOFF(0, 0, 1)] += c0;
		}
		if (INTERIOR || k >= 1) {
			const double sw = signed_by(xd0, eb.ce2);
			rowP[DOFF(0, 1, 0)] -= sw * pr0 * pm; rowP[DOFF(0, 1, 0)] -= sw * pr1 * p0;
			rowP[DOFF(0, 0, -1)] -= wlo * pr0;    rowP[DOFF(0, 0, 0)] -= wlo * pr1;
			rowR[DOFF(2, 1, 0)] -= sw * pr0 * rm; rowR[DOFF(2, 1, 0)] -= sw * pr1 * r0;
			rowR[DOFF(2, 2, -1)] -= wlo * pr0;    rowR[DOFF(2, 2, 0)] -= wlo * pr1;
		}
		if (INTERIOR || k + 1 <= L - 1) {
			const double sw = signed_by(xd1, ec.ce2);
			rowP[DOFF(0, 1, 1)] -= sw * pl0 * p0; rowP[DOFF(0, 1, 1)] -= sw * pl1 * pp;
			rowP[DOFF(0, 0, 0)] -= whi * pl0;     rowP[DOFF(0, 0, 1)] -= whi * pl1;
			rowR[DOFF(2, 1, 1)] -= sw * pl0 * r0; rowR[DOFF(2, 1, 1)] -= sw * pl1 * rp;
			rowR[DOFF(2, 2, 0)] -= whi * pl0;     rowR[DOFF(2, 2, 1)] -= whi * pl1;
		}
	}

	CBSTAMP(1);
	// ---- node k quantities the W rows of this block and of the next one use ----
	double ex0 = 0.0, wn0 = 0.0, xdn0 = 0.0, ke0 = 0.0;
	if (INTERIOR || (k <= L - 1 && (CARRY || k >= 1))) {
		ex0 = INTERIOR ? exner_from_rhotheta_bf(p, B.pn, rmtab) : (rmtab ? exner_from_rhotheta_lds(p, B.pn, rmtab) : exner_from_rhotheta(p, B.pn));
		wn0 += OPCL(TMX_OP_INTERP_REDGE_TO_NODE, k, 0) * eb.we; wn0 += OPCL(TMX_OP_INTERP_REDGE_TO_NODE, k, 1) * ec.we;
		xdn0 = B.ca2 * B.un + B.cb2 * B.vn + B.cx2 * wn0;
		const double ca = cc.c2a0 * B.un + cc.c2a1 * B.vn + B.ca2 * wn0, cb = cc.c2a1 * B.un + cc.c2b1 * B.vn + B.cb2 * wn0;
		ke0 = 0.5 * (ca * B.un + cb * B.vn + xdn0 * wn0);
	}
	CBSTAMP(2);
	if (INTERIOR || (k >= 1 && k <= L - 1)) {
		const double pm = A.pn, p0 = B.pn;
		double exm, wnm, xdnm, kem;
		if (CARRY) { exm = cy.ex; wnm = cy.wn; xdnm = cy.xdn; kem = cy.ke; }
		else {
			exm = rmtab ? exner_from_rhotheta_lds(p, pm, rmtab) : exner_from_rhotheta(p, pm);
			wnm = 0.0; wnm += OPCL(TMX_OP_INTERP_REDGE_TO_NODE, k - 1, 0) * ea.we; wnm += OPCL(TMX_OP_INTERP_REDGE_TO_NODE, k - 1, 1) * eb.we;
			xdnm = A.ca2 * A.un + A.cb2 * A.vn + A.cx2 * wnm;
			const double ca = cc.c2a0 * A.un + cc.c2a1 * A.vn + A.ca2 * wnm, cb = cc.c2a1 * A.un + cc.c2b1 * A.vn + A.cb2 * wnm;
			kem = 0.5 * (ca * A.un + cb * A.vn + xdnm * wnm);
		}
		(void)wnm;
		const double pe = pe0, re = re0;
		const double dnm = OPCL(TMX_OP_DIFF_NODE_TO_REDGE, k, -1), dn0 = OPCL(TMX_OP_DIFF_NODE_TO_REDGE, k, 0);
		double dpe = 0.0; dpe += dnm * exm; dpe += dn0 * ex0;
		const double unm = A.un, un0 = B.un, vnm = A.vn, vn0 = B.vn;
		const double wem = ea.we, we0 = eb.we, wep = ec.we;
		double dke = 0.0; dke += dnm * kem; dke += dn0 * ke0;
		double dua = 0.0; dua += dnm * unm; dua += dn0 * un0;
		double dub = 0.0; dub += dnm * vnm; dub += dn0 * vn0;
		const double ue = ue_b, ve = ve_b;
		const double cx0e = eb.ce0, cx1e = eb.ce1, cx2e = eb.ce2;
		const double xde = xd0;
		fW = dpe * pe / re;
		fW += p.grav * cc.drx;
		{
			const double ca = cc.c2a0 * ue + cc.c2a1 * ve + cx0e * we0;
			const double cb = cc.c2a1 * ue + cc.c2b1 * ve + cx1e * we0;
			const double curl = -ca * dua - cb * dub;
			fW += (dke + curl);
		}
		if (UD) fW -= udW;
		const double ddm = OPCL(TMX_OP_DIFFDIFF_REDGE_TO_REDGE, k, -1), dd0 = OPCL(TMX_OP_DIFFDIFF_REDGE_TO_REDGE, k, 0), ddp = OPCL(TMX_OP_DIFFDIFF_REDGE_TO_REDGE, k, 1);
		double ddw = 0.0; ddw += ddm * wem; ddw += dd0 * we0; ddw += ddp * wep;
		fW -= cc.upc * fabs(xde) * ddw;
		const double cA = pe * p.Rd / (re * cc.cv);
		rowW[DOFF(1, 0, -1)] += cA * dnm * exm / pm;
		rowW[DOFF(1, 0, 0)] += cA * dn0 * ex0 / p0;
		const double cB = 1.0 / (re * re) * dpe;
		{
			const double cC = cB * ib_m;
			rowW[DOFF(1, 0, -1)] += cC * re;
			rowW[DOFF(1, 2, -1)] += -cC * pe;
		}
		{
			const double cC = cB * ib_0;
			rowW[DOFF(1, 0, 0)] += cC * re;
			rowW[DOFF(1, 2, 0)] += -cC * pe;
		}
		rowW[DOFF(1, 1, -1)] += OPCL(TMX_OP_INTERP_REDGE_TO_NODE, k - 1, 0) * dnm * xdnm;
		rowW[DOFF(1, 1, 0)] += OPCL(TMX_OP_INTERP_REDGE_TO_NODE, k - 1, 1) * dnm * xdnm;
		rowW[DOFF(1, 1, 0)] += OPCL(TMX_OP_INTERP_REDGE_TO_NODE, k, 0) * dn0 * xdn0;
		rowW[DOFF(1, 1, 1)] += OPCL(TMX_OP_INTERP_REDGE_TO_NODE, k, 1) * dn0 * xdn0;
		const double sw = signed_by(xde, cx2e);
		rowW[DOFF(1, 1, 0)] -= cc.upc * sw * ddw;
		rowW[DOFF(1, 1, -1)] -= cc.upc * fabs(xde) * ddm;
		rowW[DOFF(1, 1, 0)] -= cc.upc * fabs(xde) * dd0;
		rowW[DOFF(1, 1, 1)] -= cc.upc * fabs(xde) * ddp;
	}
	CBSTAMP(3);
	rowP[4] += cc.invdt; rowW[4] += cc.invdt; rowR[4] += cc.invdt;
	if (CARRY) {
		cy.ex = ex0; cy.wn = wn0; cy.xdn = xdn0; cy.ke = ke0;
		cy.ue = ue_c; cy.ve = ve_c; cy.xd = xd1; cy.pe = pe1; cy.re = re1;
	}
#undef CBSTAMP
}
