// tmx_k_tracer_solve.hip -- the implicit column update of the tracers: hand-written CDNA4 (gfx950) kernel and its launchers (layout,
// addressing and shared helpers: tmx_device.h; the explicit column update, which holds no band LU: tmx_k_vertical.hip).
//
// Compiled with -ffp-contract=off so the arithmetic follows the operation order of the reference (built without FMA contraction).
// Reference behaviour restated (file:line under the reference tree) is cited per kernel.
#include "tmx_device.h"

// Both flavours of the band LU live in ONE library.  The rule: a translation unit whose kernels use LU_UPD (tmx_device.h) is compiled twice
// -- as it stands (LU updates fused, what OpenBLAS and MKL's FMA code paths compute) and with -DTMX_LU_NOFMA (multiply and subtract rounded
// separately, a BLAS without fused multiply-adds) -- into a namespace each; tmx_lu_select.hip dispatches by the engine's option "lu_fma"
// (tmx_set_option, any time).  This unit holds k_vi_tracers_rows (dgbtf2 / dgbtrs of the tridiagonal tracer matrix) and is a unit of its
// own so that an edit here does not compile the column solve (tmx_k_column.hip, the other such unit) twice.
#ifdef TMX_LU_NOFMA
namespace lu_nofma {
#else
namespace lu_fma {
#endif

// VerticalDynamicsFEM::UpdateColumnTracers (VerticalDynamicsFEM.cpp:3783-4282), implicit mode, vertical order 1.  The tridiagonal
// matrix (kl = ku = 1) is the same for every tracer: factorised once per column with the dgbtf2 loops (first-maximum pivoting), then
// dgbtrs per tracer (forward substitution with the stored multipliers and interchanges, column-oriented dtbsv) -- what dgbtrf + dgbtrs
// per tracer compute, and what oracle/tmx_oracle.c:orc_dgbsv, the separately written factorisation the tests compare with, pins
// against LAPACK.
// xin: initial instance (U, V, tracer densities), w0: W of the initial column [L+1][NS] (a saved copy when the step
// runs in place and the state kernel has already overwritten it), xup: update instance (updated W; receives the tracers),
// xbase: instance holding the tracer values the update is subtracted from (the update instance itself in the
// reference; the initial instance when the preceding CopyData was fused away).
// A workgroup = LW = 1 << LWB columns x NR row lanes.  Row lane t of a column evaluates xi_dot, the matrix rows, the tracer loads, the
// right-hand side and the result stores of the levels k = t, t + NR, ...; every matrix entry and every right-hand-side entry is
// formed by the lane that owns its row, in the order a sequential loop over the interfaces accumulates it (flux terms, upwinding
// of interface k then k + 1, 1/dt; velocity correction of interface k then k + 1), so the results do not depend on NR; only the
// factorisation and the two substitutions stay on one lane per column (pivot row / running entries in registers, the
// next row prefetched from LDS).  NR = 1 is that arithmetic in the serial order, one lane per column (option "vt_rows" = 0: the
// cross-check of the row ownership, the barriers and the register-carried pivot row against their own serial form).
// LDS: (9L + 3) x LW doubles per workgroup (vt_solve_lds), so that at L = 30 five workgroups of 16 columns share a CU.
template <int NR, int LWB> __global__ __launch_bounds__(NR << LWB) void k_vi_tracers_rows(KParams p, int nt, const double * __restrict__ xin, const double * __restrict__ w0,
	const double * xbase, double * xup, double dt, int nunique, const int * __restrict__ ucol, const int * __restrict__ udep, int * __restrict__ flag)
{
	constexpr int LW = 1 << LWB;        // columns per workgroup
	extern __shared__ double smt[];
	const int L = p.L, lane = threadIdx.x & (LW - 1), t = threadIdx.x >> LWB;
	const size_t NS = (size_t)p.NS;
	double * A = smt;                                // [L][4][LW]
	double * F = A + (size_t)L * 4 * LW;             // [L][LW]
	double * xd0 = F + (size_t)L * LW;               // [L+1][LW]
	double * xd1 = xd0 + (size_t)(L + 1) * LW;       // [L+1][LW]
	double * qn = xd1 + (size_t)(L + 1) * LW;        // [L][LW]
	double * jmp = qn + (size_t)L * LW;              // [L+1][LW] upwind sign x metric x (W updated - W initial) per interface
	const int uraw = blockIdx.x * LW + lane;
	const bool valid = uraw < nunique;
	const int u = valid ? uraw : nunique - 1;        // lanes of a ragged last workgroup redo the last column (no stores): barriers below
	const int col = ucol ? ucol[u] : u;
	const MetCol mc = met_col(p, col);
	const double jn = p.g2d[G2_JN * NS + col], je = p.g2d[G2_JE * NS + col];
	// row k of the band matrix in slots 0..2 (sub-, main, super-diagonal); after the factorisation: slot 0 of row j + 1 = the
	// multiplier of step j, slots 1..3 of row j = row j of U (diagonal and the two entries right of it)
#define AR(k_, s_) A[((size_t)(k_) * 4 + (s_)) * LW + lane]
	// xi_dot on interfaces, initial and with the updated W (:3943-3957, :4059-4086)
	for (int k = t; k <= L; k += NR) {
		double x0v = 0.0, x1v = 0.0, jv = 0.0;
		if (k >= 1 && k <= L - 1) {
			const double ue = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, k, [&](int off) { return xin[(size_t)TMX_SLAB_U(L, k + off) * NS + col]; });
			const double ve = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, k, [&](int off) { return xin[(size_t)TMX_SLAB_V(L, k + off) * NS + col]; });
			double e0, e1, e2;
			metric_edge(p, mc, k, col, e0, e1, e2);
			const double wi = w0[(size_t)k * NS + col], wu = xup[(size_t)TMX_SLAB_W(L, k) * NS + col];
			x0v = e0 * ue + e1 * ve + e2 * wi;
			x1v = e0 * ue + e1 * ve + e2 * wu;
			const double sw = (x0v > 0.0) ? 1.0 * e2 : ((x0v < 0.0) ? -1.0 * e2 : 0.0);
			jv = sw * (wu - wi);
		}
		xd0[(size_t)k * LW + lane] = x0v; xd1[(size_t)k * LW + lane] = x1v; jmp[(size_t)k * LW + lane] = jv;
	}
	__syncthreads();
	// matrix rows (:3959-4016), each entry by the owner of its row
	for (int k = t; k < L; k += NR) {
#pragma unroll
		for (int d = -1; d <= 1; d++) {
			const int n = k + d;
			if (n < 0 || n >= L) { AR(k, d + 1) = 0.0; continue; }
			double a = 0.0;
			// d F_k / d q_n: DiffREdgeToNode x J_e / J_n x InterpNodeToREdge x xi_dot; interface m = k + mo, node n = m + no
#pragma unroll
			for (int mo = 0; mo <= 1; mo++) {
				const int m = k + mo, no = n - m;
				if (no < -2 || no > 1) continue;
				a += OPC(TMX_OP_DIFF_REDGE_TO_NODE, k, mo) * je / jn * OPC(TMX_OP_INTERP_NODE_TO_REDGE, m, no) * xd0[(size_t)m * LW + lane];
			}
			// upwinding: interface a = k (this row as "a"), then a = k + 1 (this row as "a - 1")
			if (k >= 1 && k <= L - 1) {
				const double wgt = fabs(xd0[(size_t)k * LW + lane]);
				if (d == -1) a -= wgt * OPC(TMX_OP_PENALTY_RIGHT, k, -1);
				if (d == 0) a -= wgt * OPC(TMX_OP_PENALTY_RIGHT, k, 0);
			}
			if (k + 1 <= L - 1) {
				const double wgt = fabs(xd0[(size_t)(k + 1) * LW + lane]);
				if (d == 0) a -= wgt * OPC(TMX_OP_PENALTY_LEFT, k, 0);
				if (d == 1) a -= wgt * OPC(TMX_OP_PENALTY_LEFT, k, 1);
			}
			if (d == 0) a += 1.0 / dt;
			AR(k, d + 1) = a;
		}
	}
	__syncthreads();
	// dgbtf2 (kl = ku = 1, kv = 2), one lane per column, with the pivot candidate row carried in registers: at step j the
	// candidate has entries (c0, c1) in columns j, j + 1 (the fill-in column j + 2 holds the zero dgbtf2 stores there); row j + 1
	// is (l, d, u) in columns j .. j + 2.  Interchange when |l| > |c0| (idamax keeps the first of equals), multiplier = the other
	// row's leading entry x (1 / pivot) (dscal), rank-1 update fused as in LU_UPD, skipped for a zero in the pivot row (dger).
	bool singular = false;
	unsigned long long jpmask = 0, jpmask_hi = 0, zeromask = 0, zeromask_hi = 0;
	if (t == 0) {
		double c0 = AR(0, 1), c1 = AR(0, 2);
		double nl = (L > 1) ? AR(1, 0) : 0.0, nd = (L > 1) ? AR(1, 1) : 0.0, nu = (L > 1) ? AR(1, 2) : 0.0;
		for (int jj = 0; jj < L - 1; jj++) {
			const double l = nl, d = nd, un = nu;
			if (jj + 2 < L) { nl = AR(jj + 2, 0); nd = AR(jj + 2, 1); nu = AR(jj + 2, 2); }
			const bool jp = fabs(l) > fabs(c0);
			const double piv = jp ? l : c0;
			if (piv != 0.0) {
				const double p1 = jp ? d : c1, p2 = jp ? un : 0.0;          // pivot row right of the diagonal
				const double o0 = jp ? c0 : l, o1 = jp ? c1 : d, o2 = jp ? 0.0 : un;
				if (jp) { jpmask |= 1ull << (jj & 63); if (jj >= 64) jpmask_hi |= 1ull << (jj - 64); }
				const double r = 1.0 / piv;
				const double m = o0 * r;
				AR(jj, 1) = piv; AR(jj, 2) = p1; AR(jj, 3) = p2; AR(jj + 1, 0) = m;
				c0 = (p1 != 0.0) ? LU_UPD(o1, m, p1) : o1;
				c1 = (jp && p2 != 0.0) ? LU_UPD(o2, m, p2) : o2;
			} else {
				singular = true; zeromask |= 1ull << (jj & 63); if (jj >= 64) zeromask_hi |= 1ull << (jj - 64);
				AR(jj, 1) = c0; AR(jj, 2) = c1; AR(jj, 3) = 0.0;       // l == c0 == 0: nothing eliminated, row j + 1 becomes the candidate
				c0 = d; c1 = un;
			}
		}
		AR(L - 1, 1) = c0; AR(L - 1, 2) = 0.0; AR(L - 1, 3) = 0.0;
		if (c0 == 0.0) { singular = true; zeromask |= 1ull << ((L - 1) & 63); if (L - 1 >= 64) zeromask_hi |= 1ull << (L - 1 - 64); }
	}
	int dep[3];
#pragma unroll
	for (int q = 0; q < 3; q++) dep[q] = udep ? udep[u * 3 + q] : -1;
	for (int c = 0; c < nt; c++) {
		__syncthreads();        // the previous tracer's stores have read F
		for (int k = t; k < L; k += NR) qn[(size_t)k * LW + lane] = xin[(size_t)TMX_SLAB_Q(L, c, k) * NS + col];
		__syncthreads();
		for (int k = t; k < L; k += NR) {
			// mass flux with the updated xi_dot, its divergence (:4092-4140), upwinding with the initial xi_dot (:4153-4181): tracer_rhs_level
			auto qcol = [&](int l) { return qn[(size_t)l * LW + lane]; };
			double f = tracer_rhs_level(p.ops, L, k, je, jn, false, 0.0, qcol, qcol,
				[&](int m) { return xd1[(size_t)m * LW + lane]; }, [&](int m) { return xd0[(size_t)m * LW + lane]; }, [](int) { return 0.0; });
			// implicit velocity correction (:4183-4233): interface a = k (this row as "a"), then a = k + 1 (as "a - 1")
#pragma unroll
			for (int s_ = 0; s_ <= 1; s_++) {
				const int a = k + s_;
				if (a < 1 || a > L - 1) continue;
				const double jump = jmp[(size_t)a * LW + lane];
				if (s_ == 0) {
					f -= OPC(TMX_OP_PENALTY_RIGHT, a, -1) * qn[(size_t)(a - 1) * LW + lane] * jump;
					f -= OPC(TMX_OP_PENALTY_RIGHT, a, 0) * qn[(size_t)a * LW + lane] * jump;
				} else {
					f -= OPC(TMX_OP_PENALTY_LEFT, a - 1, 0) * qn[(size_t)(a - 1) * LW + lane] * jump;
					f -= OPC(TMX_OP_PENALTY_LEFT, a - 1, 1) * qn[(size_t)a * LW + lane] * jump;
				}
			}
			F[(size_t)k * LW + lane] = f;
		}
		__syncthreads();
		if (t == 0) {
			// dgbtrs: forward substitution with the stored multipliers and interchanges, the running entry in a register ...
			double fc = F[lane], fn = (L > 1) ? F[(size_t)LW + lane] : 0.0, mm = (L > 1) ? AR(1, 0) : 0.0;
			for (int jj = 0; jj < L - 1; jj++) {
				const double f1 = fn, m = mm;
				if (jj + 2 < L) { fn = F[(size_t)(jj + 2) * LW + lane]; mm = AR(jj + 2, 0); }
				const unsigned long long bit = 1ull << (jj & 63);
				const bool isz = (jj < 64) ? (zeromask & bit) != 0 : (zeromask_hi & (1ull << (jj - 64))) != 0;
				const bool jp = (jj < 64) ? (jpmask & bit) != 0 : (jpmask_hi & (1ull << (jj - 64))) != 0;
				const double top = (jp && !isz) ? f1 : fc, bot = (jp && !isz) ? fc : f1;
				F[(size_t)jj * LW + lane] = top;
				fc = isz ? bot : LU_UPD(bot, top, m);
			}
			// ... then dtbsv (upper, no transpose, non-unit), column oriented: entry j is divided by the diagonal and then leaves
			// entries j - 1 and j - 2; entry i therefore receives column i + 2 before column i + 1.  b1 = entry j - 1 so far.
			double cur = fc, b1 = (L > 1) ? F[(size_t)(L - 2) * LW + lane] : 0.0;
			double dg = AR(L - 1, 1), u1 = (L > 1) ? AR(L - 2, 2) : 0.0, u2 = (L > 2) ? AR(L - 3, 3) : 0.0, fr = (L > 2) ? F[(size_t)(L - 3) * LW + lane] : 0.0;
			for (int jj = L - 1; jj >= 0; jj--) {
				const double dgj = dg, u1j = u1, u2j = u2, b2 = fr;
				if (jj >= 1) dg = AR(jj - 1, 1);
				if (jj >= 2) u1 = AR(jj - 2, 2);
				if (jj >= 3) { u2 = AR(jj - 3, 3); fr = F[(size_t)(jj - 3) * LW + lane]; }
				const bool nz = cur != 0.0;
				const double x = nz ? cur / dgj : cur;
				F[(size_t)jj * LW + lane] = x;
				cur = nz ? LU_UPD(b1, x, u1j) : b1;
				b1 = nz ? LU_UPD(b2, x, u2j) : b2;
			}
		}
		__syncthreads();
		if (valid)
			for (int k = t; k < L; k += NR) {
				const size_t so = (size_t)TMX_SLAB_Q(L, c, k) * NS;
				const double val = xbase[so + col] - F[(size_t)k * LW + lane];
				xup[so + col] = val;
#pragma unroll
				for (int q = 0; q < 3; q++) if (dep[q] >= 0) xup[so + dep[q]] = val;
			}
	}
	if (singular && valid) atomicOr(flag, TMX_FLAG_SINGULAR);
#undef AR
}

// The columns a launch updates: all of them (ucol == nullptr), or the unique ones with up to three dependents each that receive a copy
struct ColumnSet { int ncols; const int * ucol, * udep; };

// The implicit column update of the tracers on a set of columns; the shape comes from vt_solve_shape_at (tmx_internal.h, with the LDS working set
// vt_solve_lds).  Option "vt_rows" (default 1), where the 16-column working set fits the
// 160 KB of a CU (L <= 141): NR row lanes per column -- 16 (four wavefronts per 16 columns) up to 48 levels, 32 above (option
// "vt_row_lanes" = 4 | 8 | 16 | 32) -- and 8 columns per workgroup up to 48 levels (half the LDS per workgroup, twice the workgroups per
// CU), 16 above (option "vt_lw8" = 0 | 1).  Fewer columns per workgroup = more workgroups per CU: the kernel lives in LDS (dependent
// read-modify-write chains of ~100 cycles each), and with 16 columns per workgroup five wavefronts share a CU and hide each other's LDS
// latency.  Else ("vt_rows" = 0, or too many levels): one row lane per column, `lanes` = 8 | 16 | 32 | 64 columns per workgroup,
// reduced to the largest power of two whose working set fits a CU (64 up to L = 35, 32 up to 70, 16 up to 141, 8 up to 284).
// Returns -1 where no shape fits (every caller has asked tmx_vertical_fit before its first kernel).
static int launch_vt_solve(tmx_engine * e, const KParams & p, const ColumnSet & cs, const double * xin, const double * w0, const double * xbase, double * xup,
	double dt, int lanes)
{
	const VtShape shape = vt_solve_shape_at(p.L, e->opt_vt_rows, e->opt_vt_nr, e->opt_vt_lw8, lanes);
	if (!shape.fits()) return -1;
	const int nr = shape.nr, lwb = shape.lwb;
	const size_t lds = shape.bytes;
	e->vt_kernel_launched = nr | lwb << 8 | (cs.ucol ? 0 : 1) << 16;      // (tmx_info(TMX_INFO_TRACER_COLUMN_KERNEL))
#define VT_SOLVE(NR_, LWB_) if (nr == NR_ && lwb == LWB_) { \
		(void)hipFuncSetAttribute((const void *)k_vi_tracers_rows<NR_, LWB_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
		hipLaunchKernelGGL((k_vi_tracers_rows<NR_, LWB_>), dim3((cs.ncols + (1 << LWB_) - 1) >> LWB_), dim3(NR_ << LWB_), lds, e->stream, p, e->nt, xin, w0, xbase, xup, dt, \
			cs.ncols, cs.ucol, cs.udep, e->d_flag); \
		return 0; }
	VT_SOLVE(8, 3) VT_SOLVE(16, 3) VT_SOLVE(32, 3)
	VT_SOLVE(4, 4) VT_SOLVE(8, 4) VT_SOLVE(16, 4) VT_SOLVE(32, 4)
	VT_SOLVE(1, 3) VT_SOLVE(1, 4) VT_SOLVE(1, 5) VT_SOLVE(1, 6)
#undef VT_SOLVE
	return -1;
}

// UpdateColumnTracers behind the implicit column solve: the unique columns, their dependents written along (option "vt_lanes", default 16)
int tmxk_vi_tracers(tmx_engine * e, const KParams & p, const double * xin, const double * w0, const double * xbase, double * xup, double dt) {
	if (e->nunique == 0 || e->nt == 0) return 0;
	return launch_vt_solve(e, p, ColumnSet{ e->nunique, (const int *)e->d_ucol, (const int *)e->d_udep }, xin, w0, xbase, xup, dt, e->opt_vt_lanes);
}

// UpdateColumnTracers at the end of StepImplicitTermsExplicitly (VerticalDynamicsFEM.cpp:600-608): the implicit column update
// of the tracers, on every stored column (the reference loops over all nodes there, :541-542), in place on the update instance
int tmxk_vi_tracers_all(tmx_engine * e, const KParams & p, const double * xin, double * xup, double dt) {
	if (e->nt == 0 || p.ncol == 0) return 0;
	return launch_vt_solve(e, p, ColumnSet{ p.ncol, nullptr, nullptr }, xin, xin + (size_t)TMX_SLAB_W(p.L, 0) * p.NS, xup, xup, dt, 64);
}

}      // namespace lu_fma / lu_nofma
