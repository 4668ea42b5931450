// tmx_k_vertical.hip -- hand-written CDNA4 (gfx950) kernels of the spectral-element hot path (one translation unit per operator family;
// layout, addressing and shared helpers: tmx_device.h).
//
// HBM layout: every field is a stack of "slabs" of NS doubles, one slab per
// (variable, level); inside a slab the index is the column  col = element*16 + i*4 + j
// (i = alpha node, j = beta node of the 4x4 GLL element).  One wavefront = 64 consecutive
// columns = 4 whole elements at one level, so every global access of a wavefront is one
// contiguous 512-byte segment and the np x np contractions stay inside a 16-lane group.
//
// All kernels are HBM-bound fp64 stencil work: one thread per (column, level),
// horizontal contractions through LDS, vertical stencils through neighbouring slabs (served by
// L2 / Infinity Cache).  Compiled with -ffp-contract=off so the arithmetic follows the operation
// order of the reference (which is built without FMA contraction).
//
// Reference behaviour restated (file:line under the reference tree) is cited per kernel.
//
// This unit holds the vertical kernels WITHOUT a band LU, i.e. that never use LU_UPD (tmx_device.h): V.StepExplicit (k_v_explicit,
// k_v_explicit_slide), the explicit column update of the tracers (k_v_tracers_explicit_column / _tile / _slide; its "solve" is a
// division by the diagonal), the negative-tracer filter (k_v_filter_tracers) and StepImplicitTermsExplicitly (k_vi_terms_explicit,
// k_vi_terms_explicit_slide: the column solve's block-row assembly, tmx_device_column.h, evaluated for F only).  It is compiled once
// and its launchers are called directly.  The kernels that hold the LU are compiled in both of its roundings: tmx_k_column.hip (the
// column solve) and tmx_k_tracer_solve.hip (the implicit column update of the tracers), dispatched by tmx_lu_select.hip.
#include "tmx_device_column.h"

template <bool UDV>
__global__ __launch_bounds__(64 * KT_VE) void k_v_explicit(KParams p, const double * __restrict__ xin,
	double * __restrict__ xup, double dt, const double * __restrict__ xref, double cf, int ntile, int xmode)
{
	int bx, by;
	if (!xcd_column_tile(xmode, ntile, (p.L + KT_VE - 1) / KT_VE, bx, by)) return;
	const int col = (p.quads ? p.quads[bx] : bx) * 64 + threadIdx.x;
	const int k = by * KT_VE + WAVE_UNIFORM(threadIdx.y);
	if (k >= p.L || col >= p.ncol) return;
	v_explicit_point<UDV>(p, xin, xup, dt, xref, cf, col, k);
}

// The same update by a thread that walks a column (or one of `nseg` segments of it) level by level: U, V of the levels k - 2 .. k + 2
// (and, UDV, the reference's) in a sliding register window, xi_dot of every interface evaluated once (the level-parallel form evaluates
// it for the level below and again for the level above), the entering level loaded an iteration ahead, operator coefficients and
// the 1 - eta table in LDS (walk_tables_to_lds).  The interface sums and the penalty row are v_explicit_point's (edge_sum, penalty_row: tmx_device.h).
template <bool UDV, bool CLOSED>
__global__ __launch_bounds__(128) void k_v_explicit_slide(KParams p, const double * __restrict__ xin, double * __restrict__ xup, double dt,
	const double * __restrict__ xref, double cf, int ntile, int xmode, int nseg)
{
	extern __shared__ double opsl[];      // [TMX_OP_COUNT][L + 1][TMX_OPW], then 1 - eta [2 L + 1]
	const int L = p.L;
	const size_t NS = (size_t)p.NS;
	double * etal = opsl + TMX_OP_COUNT * (L + 1) * TMX_OPW;
	walk_tables_to_lds<CLOSED>(p, opsl, etal);
	__syncthreads();
	constexpr int MM = CLOSED ? 1 : 2;
	int col, k0, k1;
	if (!walk_segment(p, xmode, ntile, nseg, L, col, k0, k1)) return;
	const MetCol mc = met_col(p, col);
	auto in = [&](int l) { return l >= 0 && l < L; };
	// window: levels k - 2 .. k + 2, at the (virtual) level k = k0 - 1 the walk starts from
	double uw[5], vw[5], ur[5], vr[5];
#pragma unroll
	for (int j = 0; j < 5; j++) {
		const int l = k0 - 3 + j;
		const bool ok = in(l);
		uw[j] = ok ? xin[(size_t)TMX_SLAB_U(L, l) * NS + col] : 0.0;
		vw[j] = ok ? xin[(size_t)TMX_SLAB_V(L, l) * NS + col] : 0.0;
		ur[j] = (UDV && ok) ? xref[(size_t)TMX_SLAB_U(L, l) * NS + col] : 0.0;
		vr[j] = (UDV && ok) ? xref[(size_t)TMX_SLAB_V(L, l) * NS + col] : 0.0;
	}
	double xd_lo = 0.0, upU = 0.0, upV = 0.0;
	double wm = (k0 >= 1 && k0 <= L - 1) ? xin[(size_t)TMX_SLAB_W(L, k0) * NS + col] : 0.0;      // W on the interface of the current iteration
#pragma unroll 1
	for (int k = k0 - 1; k < k1; k++) {
		const int m = k + 1;
		// the level that enters the window after this iteration, W of the next interface, the values the next level updates
		const int ln = k + 3;
		const bool okn = in(ln) && ln <= k1 + 1;
		const double eU = okn ? xin[(size_t)TMX_SLAB_U(L, ln) * NS + col] : 0.0, eV = okn ? xin[(size_t)TMX_SLAB_V(L, ln) * NS + col] : 0.0;
		const double eUR = (UDV && okn) ? xref[(size_t)TMX_SLAB_U(L, ln) * NS + col] : 0.0, eVR = (UDV && okn) ? xref[(size_t)TMX_SLAB_V(L, ln) * NS + col] : 0.0;
		const double wn = (m + 1 >= 1 && m + 1 <= L - 1 && m + 1 <= k1) ? xin[(size_t)TMX_SLAB_W(L, m + 1) * NS + col] : 0.0;
		const double upUn = (k + 1 < k1) ? xup[(size_t)TMX_SLAB_U(L, k + 1) * NS + col] : 0.0, upVn = (k + 1 < k1) ? xup[(size_t)TMX_SLAB_V(L, k + 1) * NS + col] : 0.0;
		// xi_dot on interface m (xidot_edge): window entries 1 .. 4 are the levels m - 2 .. m + 1
		double xd_hi = 0.0;
		if (m >= 1 && m <= L - 1) {
			const double ue = edge_sum(opsl, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return uw[off + 3]; });
			const double ve = edge_sum(opsl, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return vw[off + 3]; });
			double e0, e1, e2;
			metric_edge<MM>(p, mc, m, col, e0, e1, e2, etal);
			xd_hi = e0 * ue + e1 * ve + e2 * wm;
		}
		double res[2] = { 0.0, 0.0 };
		if (k >= k0) {      // level k: window entry 2
			const double w_hi = dt * fabs(xd_hi), w_lo = dt * fabs(xd_lo);
#pragma unroll
			for (int v = 0; v < 2; v++) {
				const double * x = v ? vw : uw, * xr = v ? vr : ur;
				double out = penalty_row(opsl, L, k, v ? upV : upU, [&](int d) { return x[d + 2]; }, w_lo, w_hi);
				if (UDV) {
					double dd = 0.0, ddr = 0.0;
#pragma unroll
					for (int off = -2; off <= 2; off++) {
						const int l = k + off;
						if (l < 0 || l >= L) continue;
						const double c = OPCL(TMX_OP_DIFFDIFF_NODE_TO_NODE, k, off);
						dd += c * x[off + 2];
						ddr += c * xr[off + 2];
					}
					out += dt * cf * (dd - ddr);
				}
				res[v] = out;
			}
		}
		xd_lo = xd_hi; wm = wn; upU = upUn; upV = upVn;
#pragma unroll
		for (int j = 0; j < 4; j++) { uw[j] = uw[j + 1]; vw[j] = vw[j + 1]; ur[j] = ur[j + 1]; vr[j] = vr[j + 1]; }
		uw[4] = eU; vw[4] = eV; ur[4] = eUR; vr[4] = eVR;
		// the stores last, the entering level landed before them (see k_v_tracers_explicit_slide)
		asm volatile("" : "+v"(uw[4]), "+v"(vw[4]), "+v"(wm), "+v"(upU), "+v"(upV));
		if (UDV) asm volatile("" : "+v"(ur[4]), "+v"(vr[4]));
		if (k >= k0) { xup[(size_t)k * NS + col] = res[0]; xup[(size_t)(L + k) * NS + col] = res[1]; }
	}
}

void tmxk_v_explicit(tmx_engine * e, const KParams & p, const double * xin, double * xup, double dt, bool with_udiff_uv) {
	const int nt_ = NTILES(e, p), xm = e->xcd_vertical;
	const WalkShape shape = vwalk_shape(TMX_WALK_VX, p.L, e->opt_vx_walk, nt_);
	e->vwalk_launched[TMX_WALK_VX] = shape.nseg;      // (tmx_info(TMX_INFO_VERTICAL_KERNELS): the walk's segments, 0 the level-parallel kernel below)
	if (shape.nseg) {      // a thread walks (a segment of) its column; -n = n segments, -1000 = chosen from the grid size
		// (a light kernel, four resident wavefronts per SIMD: ne30 L40 on one GPU 1 / 2 / 4 segments 3.84 / 3.76 / 3.75 ms per step of BASELINE config 4's
		// shape, the level-parallel kernel 3.98)
		const int nseg = shape.nseg;
		const size_t lds_slide = shape.bytes;
		dim3 blk(64, 2), grd(xcd_column_grid(xm, nt_, (nseg + 1) / 2));
		const double cf = with_udiff_uv ? e->cfg.uniform_diffusion_vector / (e->cfg.ztop * e->cfg.ztop) : 0.0;
#define LAUNCH_VXS(UD_, CL_) hipLaunchKernelGGL((k_v_explicit_slide<UD_, CL_>), grd, blk, lds_slide, e->stream, p, xin, xup, dt, (const double *)(with_udiff_uv ? e->d_ref : nullptr), cf, nt_, xm, nseg)
		if (with_udiff_uv) { if (p.closed) LAUNCH_VXS(true, true); else LAUNCH_VXS(true, false); }
		else { if (p.closed) LAUNCH_VXS(false, true); else LAUNCH_VXS(false, false); }
#undef LAUNCH_VXS
		return;
	}
	dim3 blk(64, KT_VE), grd(xcd_column_grid(xm, nt_, (p.L + KT_VE - 1) / KT_VE));
	if (with_udiff_uv)
		hipLaunchKernelGGL(k_v_explicit<true>, grd, blk, 0, e->stream, p, xin, xup, dt, (const double *)e->d_ref,
			e->cfg.uniform_diffusion_vector / (e->cfg.ztop * e->cfg.ztop), nt_, xm);
	else
		hipLaunchKernelGGL(k_v_explicit<false>, grd, blk, 0, e->stream, p, xin, xup, dt, (const double *)nullptr, 0.0, nt_, xm);
}

// VerticalDynamicsFEM::UpdateColumnTracers (VerticalDynamicsFEM.cpp:3783-4282) in the fully explicit vertical mode (:3910-3912,
// :4047-4063, :4117-4141, :4166-4170, :4193), one lane per stored column, the column's operands in LDS (option "vt_column": the
// cross-check of the level-parallel and column-walking forms below).  Every stored column is advanced on its own, in place on the
// update instance (which has not been through the DSS yet); the matrix is the diagonal 1/dt (dgbtrs then is one division per level:
// tracer_explicit_solve, no band LU), xi_dot comes from the initial W for the flux and for the upwinding alike, there is no velocity
// correction, and with ks != 0 the mass flux carries the uniform diffusion of q / rho - (q / rho)_ref.
// LW = columns per workgroup (the lane stride of the LDS arrays): 64, or 32 -- half-filled wavefronts, twice the workgroups -- where
// 64 columns do not fit a CU (vt_explicit_column_lds).
template <int LW>
__global__ __launch_bounds__(64) void k_v_tracers_explicit_column(KParams p, int nt, const double * __restrict__ xin, double * xup, double dt,
	double ks, const double * __restrict__ xref)
{
	extern __shared__ double smt[];
	const int L = p.L, lane = threadIdx.x;
	const size_t NS = (size_t)p.NS;
	double * xd0 = smt;                            // [L+1][LW] xi_dot of the initial column on interfaces
	double * rhoe = xd0 + (size_t)(L + 1) * LW;    // [L+1][LW] rho on interfaces (uniform diffusion only)
	double * qn = rhoe + (size_t)(L + 1) * LW;     // [L][LW] tracer density of the column
	double * mixr = qn + (size_t)L * LW;           // [L][LW] q / rho - (q / rho)_ref (uniform diffusion only)
	const int col = blockIdx.x * LW + lane;
	if (lane >= LW || col >= p.ncol) return;
	const MetCol mc = met_col(p, col);
	const double jn = p.g2d[G2_JN * NS + col], je = p.g2d[G2_JE * NS + col];
	const double * w0 = xin + (size_t)TMX_SLAB_W(L, 0) * NS;
	// U,V on interfaces (InterpolateNodeToREdge of the initial column), xi_dot (:3943-3957)
	for (int k = 0; k <= L; k++) {
		double x0v = 0.0;
		if (k >= 1 && k <= L - 1) {
			const double ue = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, k, [&](int off) { return xin[(size_t)TMX_SLAB_U(L, k + off) * NS + col]; });
			const double ve = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, k, [&](int off) { return xin[(size_t)TMX_SLAB_V(L, k + off) * NS + col]; });
			double e0, e1, e2;
			metric_edge(p, mc, k, col, e0, e1, e2);
			x0v = e0 * ue + e1 * ve + e2 * w0[(size_t)k * NS + col];
		}
		xd0[(size_t)k * LW + lane] = x0v;
	}
	if (ks != 0.0) {
		// rho on interfaces: InterpolateNodeToREdge of the initial column (PrepareColumn :1905-1916)
		for (int m = 0; m <= L; m++)
			rhoe[(size_t)m * LW + lane] = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return xin[(size_t)TMX_SLAB_R(L, m + off) * NS + col]; });
	}
	const double idt = 1.0 / dt;
	auto xd = [&](int m) { return xd0[(size_t)m * LW + lane]; };
	for (int c = 0; c < nt; c++) {
		for (int k = 0; k < L; k++) qn[(size_t)k * LW + lane] = xin[(size_t)TMX_SLAB_Q(L, c, k) * NS + col];
		if (ks != 0.0)
			for (int k = 0; k < L; k++) {
				double a = qn[(size_t)k * LW + lane] / xin[(size_t)TMX_SLAB_R(L, k) * NS + col];
				a -= xref[(size_t)TMX_SLAB_Q(L, c, k) * NS + col] / xref[(size_t)TMX_SLAB_R(L, k) * NS + col];
				mixr[(size_t)k * LW + lane] = a;
			}
		// mass flux, its divergence (:4092-4140), upwinding (:4153-4181): tracer_rhs_level; the diagonal matrix 1/dt: dgbtrs leaves b_j / (1/dt)
		for (int k = 0; k < L; k++) {
			const double f = tracer_rhs_level(p.ops, L, k, je, jn, ks != 0.0, ks,
				[&](int l) { return qn[(size_t)l * LW + lane]; }, [&](int l) { return mixr[(size_t)l * LW + lane]; }, xd, xd, [&](int m) { return rhoe[(size_t)m * LW + lane]; });
			const size_t so = (size_t)TMX_SLAB_Q(L, c, k) * NS;
			xup[so + col] = xup[so + col] - tracer_explicit_solve(f, idt);
		}
	}
}

// 64 columns per workgroup, or 32 where only they fit the 160 KB of a CU (vt_column_shape, tmx_internal.h, with the LDS working set
// vt_explicit_column_lds); returns -1 where neither does (every caller has asked tmx_vertical_fit before its first kernel)
static int launch_vt_explicit_column(tmx_engine * e, const KParams & p, const double * xin, double * xup, double dt) {
	const VtColumnShape shape = vt_column_shape(p.L);
	if (!shape.fits()) return -1;
	const int lw = shape.lw;
	const size_t lds = shape.bytes;
	e->vwalk_launched[TMX_WALK_VT] = 0x800 | lw;      // (tmx_info(TMX_INFO_VERTICAL_KERNELS))
	const double ks = e->udiff ? e->cfg.uniform_diffusion_scalar : 0.0;
#define LAUNCH_VTC(LW_) do { (void)hipFuncSetAttribute((const void *)k_v_tracers_explicit_column<LW_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
	hipLaunchKernelGGL(k_v_tracers_explicit_column<LW_>, dim3((p.ncol + LW_ - 1) / LW_), dim3(64), lds, e->stream, p, e->nt, xin, xup, dt, ks, (const double *)e->d_ref); } while (0)
	if (lw == 64) LAUNCH_VTC(64); else LAUNCH_VTC(32);
#undef LAUNCH_VTC
	return 0;
}

#if TMX_EXP      // the form without LDS staging (option "vt_explicit_v1"), superseded by k_v_tracers_explicit_tile: experiments flavour only
// UpdateColumnTracers in the fully explicit vertical mode, level-parallel.  There the matrix is the diagonal 1/dt, so the
// update of (column, level, tracer) only needs the column within two levels: one thread per (column, level) evaluates
// the right-hand side of k_v_tracers_explicit_column (tracer_rhs_level, tmx_device.h) instead of one
// lane walking the whole column out of LDS -- that form took 3.4 ms per launch at ne30 L40 (32 columns per workgroup, 82 KB
// of LDS each), 75 % of a supercell step.
__global__ __launch_bounds__(256) void k_v_tracers_explicit(KParams p, int nt, const double * __restrict__ xin, double * xup, double dt,
	double ks, const double * __restrict__ xref)
{
	const int L = p.L;
	const size_t NS = (size_t)p.NS;
	const int col = TILE_X(p) * 64 + threadIdx.x;
	const int k = blockIdx.y * 4 + WAVE_UNIFORM(threadIdx.y);
	if (k >= L || col >= p.ncol) return;
	const MetCol mc = met_col(p, col);
	const double jn = p.g2d[G2_JN * NS + col], je = p.g2d[G2_JE * NS + col];
	const double * w0 = xin + (size_t)TMX_SLAB_W(L, 0) * NS;
	// xi_dot of the initial column on the interfaces k and k+1 (zero at the boundaries)
	double xd[2];
#pragma unroll
	for (int mo = 0; mo <= 1; mo++) {
		const int m = k + mo;
		double x0v = 0.0;
		if (m >= 1 && m <= L - 1) {
			const double ue = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return xin[(size_t)TMX_SLAB_U(L, m + off) * NS + col]; });
			const double ve = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return xin[(size_t)TMX_SLAB_V(L, m + off) * NS + col]; });
			double e0, e1, e2;
			metric_edge(p, mc, m, col, e0, e1, e2);
			x0v = e0 * ue + e1 * ve + e2 * w0[(size_t)m * NS + col];
		}
		xd[mo] = x0v;
	}
	// rho on the two interfaces (uniform diffusion only)
	double rhoe[2] = { 0.0, 0.0 };
	if (ks != 0.0) {
#pragma unroll
		for (int mo = 0; mo <= 1; mo++) rhoe[mo] = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, k + mo, [&](int off) { return xin[(size_t)TMX_SLAB_R(L, k + mo + off) * NS + col]; });
	}
	// rho of the five levels k-2 .. k+2 the stencils reach (each value is loaded once and divided once per tracer)
	double rh5[5] = { 1.0, 1.0, 1.0, 1.0, 1.0 }, rr5[5] = { 1.0, 1.0, 1.0, 1.0, 1.0 };
	if (ks != 0.0) {
#pragma unroll
		for (int t = 0; t < 5; t++) {
			const int l = k - 2 + t;
			if (l < 0 || l >= L) continue;
			rh5[t] = xin[(size_t)TMX_SLAB_R(L, l) * NS + col];
			rr5[t] = xref[(size_t)TMX_SLAB_R(L, l) * NS + col];
		}
	}
	for (int c = 0; c < nt; c++) {
		double q5[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 }, mr5[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
		for (int t = 0; t < 5; t++) {
			const int l = k - 2 + t;
			if (l < 0 || l >= L) continue;
			q5[t] = xin[(size_t)TMX_SLAB_Q(L, c, l) * NS + col];
			if (ks != 0.0) {
				double a_ = q5[t] / rh5[t];
				a_ -= xref[(size_t)TMX_SLAB_Q(L, c, l) * NS + col] / rr5[t];
				mr5[t] = a_;
			}
		}
		auto qn = [&](int l) -> double { return q5[l - k + 2]; };          // l in [k-2, k+2], unrolled: a register
		auto mixr = [&](int l) -> double { return mr5[l - k + 2]; };
		const double F = tracer_explicit_solve(tracer_rhs_level(p.ops, L, k, je, jn, ks != 0.0, ks, qn, mixr,
			[&](int m) { return xd[m - k]; }, [&](int m) { return xd[m - k]; }, [&](int m) { return rhoe[m - k]; }), 1.0 / dt);
		const size_t so = (size_t)TMX_SLAB_Q(L, c, k) * NS;
		xup[so + col] = xup[so + col] - F;
	}
}
#endif      // TMX_EXP

// The same update (k_v_tracers_explicit, experiments flavour: one thread per (column, level) with every operand from memory) with the shared operands of a tile staged once in LDS: a workgroup = 64 columns x 8 levels; xi_dot (and, with
// uniform diffusion, rho) on the tile's 9 interfaces, rho on its 12 levels and per tracer the 12 column values and mixing-ratio
// deviations (two fp64 divisions each) are evaluated by one thread each instead of by every thread whose stencil reaches them
// (5 x for the divisions: 372 -> 264 us per launch at ne30 L40 with three tracers).  The right-hand side itself is tracer_rhs_level (tmx_device.h), as in k_v_tracers_explicit_column.
__global__ __launch_bounds__(512) void k_v_tracers_explicit_tile(KParams p, int nt, const double * __restrict__ xin, double * xup, double dt,
	double ks, const double * __restrict__ xref, int ntile, int xmode)
{
	constexpr int KT = 8, NL = KT + 4, NI = KT + 1;
	__shared__ double s_xd[NI][64], s_re[NI][64], s_rh[NL][64], s_rr[NL][64], s_q[NL][64], s_mr[NL][64];
	const int L = p.L;
	const size_t NS = (size_t)p.NS;
	const int tx = threadIdx.x, y = WAVE_UNIFORM(threadIdx.y);
	int bx, by;
	if (!xcd_column_tile(xmode, ntile, (L + KT - 1) / KT, bx, by)) return;
	const int col = (p.quads ? p.quads[bx] : bx) * 64 + tx;
	const int k0 = by * KT, k = k0 + y;
	const double * w0 = xin + (size_t)TMX_SLAB_W(L, 0) * NS;
	const double jn = p.g2d[G2_JN * NS + col], je = p.g2d[G2_JE * NS + col];
	// the column values a thread stages (levels y and y + KT of the tile's 12) and the value it updates are loaded one tracer
	// ahead of their use, so that their latency overlaps the previous tracer's arithmetic instead of following a barrier
	double pq[2] = { 0.0, 0.0 }, pr[2] = { 0.0, 0.0 }, pup = 0.0;
	const bool mine = k < L && col < p.ncol;
	auto prefetch = [&](int c) {
#pragma unroll
		for (int h = 0; h < 2; h++) {
			const int li = y + h * KT, l = k0 - 2 + li;
			if (li < NL && l >= 0 && l < L) {
				pq[h] = xin[(size_t)TMX_SLAB_Q(L, c, l) * NS + col];
				if (ks != 0.0) pr[h] = xref[(size_t)TMX_SLAB_Q(L, c, l) * NS + col];
			}
		}
		if (mine) pup = xup[(size_t)TMX_SLAB_Q(L, c, k) * NS + col];
	};
	if (nt > 0) prefetch(0);       // in flight while the shared operands below are staged
	{
		const MetCol mc = met_col(p, col);
		for (int mi = y; mi < NI; mi += KT) {
			const int m = k0 + mi;
			double x0v = 0.0, re = 0.0;
			if (m >= 1 && m <= L - 1) {
				const double ue = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return xin[(size_t)TMX_SLAB_U(L, m + off) * NS + col]; });
				const double ve = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return xin[(size_t)TMX_SLAB_V(L, m + off) * NS + col]; });
				double e0, e1, e2;
				metric_edge(p, mc, m, col, e0, e1, e2);
				x0v = e0 * ue + e1 * ve + e2 * w0[(size_t)m * NS + col];
			}
			if (ks != 0.0 && m <= L) re = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return xin[(size_t)TMX_SLAB_R(L, m + off) * NS + col]; });
			s_xd[mi][tx] = x0v; s_re[mi][tx] = re;
		}
		for (int li = y; li < NL; li += KT) {
			const int l = k0 - 2 + li;
			double a = 1.0, b = 1.0;
			if (ks != 0.0 && l >= 0 && l < L) { a = xin[(size_t)TMX_SLAB_R(L, l) * NS + col]; b = xref[(size_t)TMX_SLAB_R(L, l) * NS + col]; }
			s_rh[li][tx] = a; s_rr[li][tx] = b;
		}
	}
	for (int c = 0; c < nt; c++) {
		__syncthreads();           // first pass: the staging above; later passes: the previous tracer's reads of s_q / s_mr
#pragma unroll
		for (int h = 0; h < 2; h++) {
			const int li = y + h * KT, l = k0 - 2 + li;
			if (li >= NL) continue;
			double qv = 0.0, mr = 0.0;
			if (l >= 0 && l < L) {
				qv = pq[h];
				if (ks != 0.0) {
					double a_ = qv / s_rh[li][tx];
					a_ -= pr[h] / s_rr[li][tx];
					mr = a_;
				}
			}
			s_q[li][tx] = qv; s_mr[li][tx] = mr;
		}
		const double up0 = pup;
		if (c + 1 < nt) prefetch(c + 1);
		__syncthreads();
		if (k >= L || col >= p.ncol) continue;
		auto qn = [&](int l) -> double { return s_q[l - k0 + 2][tx]; };
		auto mixr = [&](int l) -> double { return s_mr[l - k0 + 2][tx]; };
		const double F = tracer_explicit_solve(tracer_rhs_level(p.ops, L, k, je, jn, ks != 0.0, ks, qn, mixr,
			[&](int m) { return s_xd[m - k0][tx]; }, [&](int m) { return s_xd[m - k0][tx]; }, [&](int m) { return s_re[m - k0][tx]; }), 1.0 / dt);
		const size_t so = (size_t)TMX_SLAB_Q(L, c, k) * NS;
		xup[so + col] = up0 - F;
	}
}

#if TMX_EXP      // superseded by the sliding-window form below (measured: -2 % against the tiled kernel at 4 levels per thread, slower at 8 and 10): experiments flavour only
// The same update by column segments: a thread = (column, KC consecutive levels), no LDS and no barrier.  The operands a segment's
// stencils reach -- U, V, rho on KC + 3 / KC + 4 levels, per tracer the KC + 4 column values and mixing-ratio deviations -- are loaded
// once into registers and every interface flux is formed once (the level-parallel forms evaluate the flux of interface k + 1 for level
// k and again for level k + 1: the same expression on the same operands, so once is the same value): tracer_edge_flux, then
// penalty_row and tracer_rhs_row (tmx_device.h), the pieces of the level-parallel forms' tracer_rhs_level.
template <int KC>
__global__ __launch_bounds__(64) void k_v_tracers_explicit_walk(KParams p, int nt, const double * __restrict__ xin, double * xup, double dt,
	double ks, const double * __restrict__ xref, int ntile, int xmode)
{
	constexpr int NL = KC + 4, NI = KC + 1;
	const int L = p.L;
	const size_t NS = (size_t)p.NS;
	int bx, by;
	if (!xcd_column_tile(xmode, ntile, (L + KC - 1) / KC, bx, by)) return;
	const int col = (p.quads ? p.quads[bx] : bx) * 64 + threadIdx.x;
	if (col >= p.ncol) return;
	const int k0 = WAVE_UNIFORM(by * KC);
	const int nk = min(KC, L - k0);
	const double * w0 = xin + (size_t)TMX_SLAB_W(L, 0) * NS;
	const double jn = p.g2d[G2_JN * NS + col], je = p.g2d[G2_JE * NS + col];
	double xd[NI], re[NI], rh[NL], rr[NL];
	{
		// xi_dot of the initial column on the segment's interfaces (zero at the boundaries), rho there (uniform diffusion only)
		const MetCol mc = met_col(p, col);
		double uw[KC + 3], vw[KC + 3];
#pragma unroll
		for (int t = 0; t < KC + 3; t++) {
			const int l = k0 - 2 + t;
			uw[t] = 0.0; vw[t] = 0.0;
			if (l >= 0 && l < L) { uw[t] = xin[(size_t)TMX_SLAB_U(L, l) * NS + col]; vw[t] = xin[(size_t)TMX_SLAB_V(L, l) * NS + col]; }
		}
#pragma unroll
		for (int li = 0; li < NL; li++) {
			const int l = k0 - 2 + li;
			rh[li] = 1.0; rr[li] = 1.0;
			if (ks != 0.0 && l >= 0 && l < L) { rh[li] = xin[(size_t)TMX_SLAB_R(L, l) * NS + col]; rr[li] = xref[(size_t)TMX_SLAB_R(L, l) * NS + col]; }
		}
#pragma unroll
		for (int mi = 0; mi < NI; mi++) {
			const int m = k0 + mi;
			double x0v = 0.0, r0 = 0.0;
			if (mi <= nk && m >= 1 && m <= L - 1) {
				const double ue = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return uw[mi + off + 2]; });
				const double ve = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return vw[mi + off + 2]; });
				double e0, e1, e2;
				metric_edge(p, mc, m, col, e0, e1, e2);
				x0v = e0 * ue + e1 * ve + e2 * w0[(size_t)m * NS + col];
			}
			if (ks != 0.0 && mi <= nk && m <= L) r0 = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return rh[mi + off + 2]; });
			xd[mi] = x0v; re[mi] = r0;
		}
	}
	const double idt = 1.0 / dt;
	for (int c = 0; c < nt; c++) {
		double q[NL], mr[NL], up0[KC];
#pragma unroll
		for (int li = 0; li < NL; li++) {
			const int l = k0 - 2 + li;
			double qv = 0.0, a_ = 0.0;
			if (l >= 0 && l < L) {
				qv = xin[(size_t)TMX_SLAB_Q(L, c, l) * NS + col];
				if (ks != 0.0) {
					a_ = qv / rh[li];
					a_ -= xref[(size_t)TMX_SLAB_Q(L, c, l) * NS + col] / rr[li];
				}
			}
			q[li] = qv; mr[li] = a_;
		}
#pragma unroll
		for (int i = 0; i < KC; i++) up0[i] = (i < nk) ? xup[(size_t)TMX_SLAB_Q(L, c, k0 + i) * NS + col] : 0.0;
		double mf[NI];
#pragma unroll
		for (int mi = 0; mi < NI; mi++) {
			const int m = k0 + mi;
			double v = 0.0;
			if (mi <= nk) v = tracer_edge_flux(p.ops, L, m, je, xd[mi], ks != 0.0, ks, re[mi], [&](int off) { return q[mi + off + 2]; }, [&](int off) { return mr[mi + off + 2]; });
			mf[mi] = v;
		}
#pragma unroll
		for (int i = 0; i < KC; i++) {
			if (i >= nk) continue;
			const int k = k0 + i;
			const double aux = penalty_row(p.ops, L, k, 0.0, [&](int d) { return q[i + d + 2]; }, fabs(xd[i]), fabs(xd[i + 1]));
			const double F = tracer_explicit_solve(tracer_rhs_row(p.ops, L, k, mf[i], mf[i + 1], jn, aux), idt);
			xup[(size_t)TMX_SLAB_Q(L, c, k) * NS + col] = up0[i] - F;
		}
	}
}

#endif      // TMX_EXP

// The same update by a thread that walks a column (or one of `nseg` segments of it) level by level with the stencils' operands in a
// sliding register window -- the four levels k - 1 .. k + 2 of U, V, rho and, for NTR tracers at once, of the column values and
// mixing-ratio deviations -- so that every operand is loaded once (a segment re-reads the four levels around its ends), the two
// divisions of a deviation and every interface flux are evaluated once, and the level entering the window is loaded an iteration
// ahead of its first use.  No barrier in the walk.  The arithmetic is tracer_edge_flux, penalty_row and tracer_rhs_row (tmx_device.h).
// The operator coefficients and the 1 - eta table come from LDS (walk_tables_to_lds).
template <int NTR, bool CLOSED>
__global__ __launch_bounds__(128) void k_v_tracers_explicit_slide(KParams p, int c0, const double * __restrict__ xin, double * xup, double dt,
	double ks, const double * __restrict__ xref, int ntile, int xmode, int nseg)
{
	extern __shared__ double opsl[];      // [TMX_OP_COUNT][L + 1][TMX_OPW], then 1 - eta [2 L + 1]
	const int L = p.L;
	const size_t NS = (size_t)p.NS;
	double * etal = opsl + TMX_OP_COUNT * (L + 1) * TMX_OPW;
	walk_tables_to_lds<CLOSED>(p, opsl, etal);
	__syncthreads();
	constexpr int MM = CLOSED ? 1 : 2;
	int col, k0, k1;
	if (!walk_segment(p, xmode, ntile, nseg, L, col, k0, k1)) return;
	const double * w0 = xin + (size_t)TMX_SLAB_W(L, 0) * NS;
	const double jn = p.g2d[G2_JN * NS + col], je = p.g2d[G2_JE * NS + col];
	const MetCol mc = met_col(p, col);
	const bool ud = ks != 0.0;
	const double idt = 1.0 / dt;
	auto in = [&](int l) { return l >= 0 && l < L; };
	// deviation of the mixing ratio from the reference's (uniform diffusion only), as the staging of the tiled kernel forms it
	auto deviation = [&](bool ok, double qv, double rhv, double qrv, double rrv) -> double {
		double a_ = 0.0;
		if (ok && ud) { a_ = qv / rhv; a_ -= qrv / rrv; }
		return a_;
	};
	// window: levels k - 1 .. k + 2, at the (virtual) level k = k0 - 1 the walk starts from
	double uw[4], vw[4], rh[4], q[NTR][4], mr[NTR][4];
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const int l = k0 - 2 + j;
		const bool ok = in(l);
		uw[j] = ok ? xin[(size_t)TMX_SLAB_U(L, l) * NS + col] : 0.0;
		vw[j] = ok ? xin[(size_t)TMX_SLAB_V(L, l) * NS + col] : 0.0;
		const double rhv = (ok && ud) ? xin[(size_t)TMX_SLAB_R(L, l) * NS + col] : 1.0, rrv = (ok && ud) ? xref[(size_t)TMX_SLAB_R(L, l) * NS + col] : 1.0;
		rh[j] = rhv;
#pragma unroll
		for (int t = 0; t < NTR; t++) {
			const double qv = ok ? xin[(size_t)TMX_SLAB_Q(L, c0 + t, l) * NS + col] : 0.0;
			const double qrv = (ok && ud) ? xref[(size_t)TMX_SLAB_Q(L, c0 + t, l) * NS + col] : 0.0;
			q[t][j] = qv; mr[t][j] = deviation(ok, qv, rhv, qrv, rrv);
		}
	}
	double xd_lo = 0.0, mf_lo[NTR], up[NTR];
#pragma unroll
	for (int t = 0; t < NTR; t++) { mf_lo[t] = 0.0; up[t] = 0.0; }
	double wm = (k0 >= 1 && k0 <= L - 1) ? w0[(size_t)k0 * NS + col] : 0.0;      // W on the interface of the current iteration
	for (int k = k0 - 1; k < k1; k++) {
		const int m = k + 1;
		// the level that enters the window after this iteration, W of the next interface, the values the next level updates
		const int ln = k + 3;
		const bool okn = in(ln) && ln <= k1 + 1;
		const double eU = okn ? xin[(size_t)TMX_SLAB_U(L, ln) * NS + col] : 0.0, eV = okn ? xin[(size_t)TMX_SLAB_V(L, ln) * NS + col] : 0.0;
		const double eR = (okn && ud) ? xin[(size_t)TMX_SLAB_R(L, ln) * NS + col] : 1.0, eRR = (okn && ud) ? xref[(size_t)TMX_SLAB_R(L, ln) * NS + col] : 1.0;
		const double wn = (m + 1 >= 1 && m + 1 <= L - 1 && m + 1 <= k1) ? w0[(size_t)(m + 1) * NS + col] : 0.0;
		double eQ[NTR], eQR[NTR], upn[NTR];
#pragma unroll
		for (int t = 0; t < NTR; t++) {
			eQ[t] = okn ? xin[(size_t)TMX_SLAB_Q(L, c0 + t, ln) * NS + col] : 0.0;
			eQR[t] = (okn && ud) ? xref[(size_t)TMX_SLAB_Q(L, c0 + t, ln) * NS + col] : 0.0;
			upn[t] = (k + 1 < k1) ? xup[(size_t)TMX_SLAB_Q(L, c0 + t, k + 1) * NS + col] : 0.0;
		}
		// xi_dot (zero at the boundaries) and, with uniform diffusion, rho on interface m
		double xd_hi = 0.0, re_hi = 0.0;
		if (m >= 1 && m <= L - 1) {
			const double ue = edge_sum(opsl, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return uw[off + 2]; });
			const double ve = edge_sum(opsl, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return vw[off + 2]; });
			double e0, e1, e2;
			metric_edge<MM>(p, mc, m, col, e0, e1, e2, etal);
			xd_hi = e0 * ue + e1 * ve + e2 * wm;
		}
		if (ud && m <= L) re_hi = edge_sum(opsl, L, TMX_OP_INTERP_NODE_TO_REDGE, m, [&](int off) { return rh[off + 2]; });
		double res[NTR];
#pragma unroll
		for (int t = 0; t < NTR; t++) {
			// window entries 0 .. 3 are the levels m - 2 .. m + 1 = k - 1 .. k + 2
			const double mf_hi = tracer_edge_flux(opsl, L, m, je, xd_hi, ud, ks, re_hi, [&](int off) { return q[t][off + 2]; }, [&](int off) { return mr[t][off + 2]; });
			if (k >= k0) {
				const double aux = penalty_row(opsl, L, k, 0.0, [&](int d) { return q[t][d + 1]; }, fabs(xd_lo), fabs(xd_hi));
				res[t] = up[t] - tracer_explicit_solve(tracer_rhs_row(opsl, L, k, mf_lo[t], mf_hi, jn, aux), idt);
			} else res[t] = 0.0;
			mf_lo[t] = mf_hi;
			// the window moves up one level
			q[t][0] = q[t][1]; q[t][1] = q[t][2]; q[t][2] = q[t][3]; q[t][3] = eQ[t];
			mr[t][0] = mr[t][1]; mr[t][1] = mr[t][2]; mr[t][2] = mr[t][3]; mr[t][3] = deviation(okn, eQ[t], eR, eQR[t], eRR);
			up[t] = upn[t];
		}
		xd_lo = xd_hi; wm = wn;
		uw[0] = uw[1]; uw[1] = uw[2]; uw[2] = uw[3]; uw[3] = eU;
		vw[0] = vw[1]; vw[1] = vw[2]; vw[2] = vw[3]; vw[3] = eV;
		rh[0] = rh[1]; rh[1] = rh[2]; rh[2] = rh[3]; rh[3] = eR;
		// The level's stores LAST, behind everything that reads a value loaded in this iteration: the stores sit in a branch, the compiler
		// cannot count them, and a loaded value first used behind them waits for everything in flight (s_waitcnt vmcnt(0)) -- i.e. for the
		// stores' own completion, once per tracer and level (the entering level's values are made to land first: the empty asm statements).
		asm volatile("" : "+v"(uw[3]), "+v"(vw[3]), "+v"(wm));
#pragma unroll
		for (int t = 0; t < NTR; t++) asm volatile("" : "+v"(q[t][3]), "+v"(mr[t][3]), "+v"(up[t]));
		if (k >= k0) {
#pragma unroll
			for (int t = 0; t < NTR; t++) xup[(size_t)TMX_SLAB_Q(L, c0 + t, k) * NS + col] = res[t];
		}
	}
}

// UpdateColumnTracers in the fully explicit vertical mode: every stored column, in place on the update instance
int tmxk_vi_tracers_explicit(tmx_engine * e, const KParams & p, const double * xin, double * xup, double dt) {
	if (e->nt == 0 || p.ncol == 0) return 0;
	if (!e->opt_vt_column) {      // level-parallel / column-walking forms; option "vt_column": the one-lane-per-column LDS kernel, for A/B and tests
		const WalkShape shape = vwalk_shape(TMX_WALK_VT, p.L, e->opt_vt_walk, NTILES(e, p));
		e->vwalk_launched[TMX_WALK_VT] = 0;      // (tmx_info(TMX_INFO_VERTICAL_KERNELS): the walk's segments, 0 every other form below)
#if TMX_EXP
		if (e->opt_vt_explicit_v1) {      // the form without LDS staging, for A/B and tests
			dim3 blk(64, 4), grd(NTILES(e, p), (p.L + 3) / 4);
			hipLaunchKernelGGL(k_v_tracers_explicit, grd, blk, 0, e->stream, p, e->nt, xin, xup, dt,
				e->udiff ? e->cfg.uniform_diffusion_scalar : 0.0, (const double *)e->d_ref);
		} else
#endif
		if (shape.nseg) {      // a thread walks (a segment of) its column: -n = n segments per column
			const int nt_ = NTILES(e, p), xm = e->xcd_vertical;
			e->vwalk_launched[TMX_WALK_VT] = shape.nseg;
			// default (-1000): segments in pairs (the two wavefronts of a workgroup) until the chip has two wavefronts per SIMD, at least five
			// levels each -- ne30 L40 on one GPU: 1 350 tiles x 2 (measured: 1 / 2 / 3 / 4 segments 4.27 / 4.08 / 4.28 / 4.20 ms per step of BASELINE
			// config 4's shape, the LDS-tiled kernel 4.67)
			const int nseg = shape.nseg;
			dim3 blk(64, 2), grd(xcd_column_grid(xm, nt_, (nseg + 1) / 2));
			const double ks_ = e->udiff ? e->cfg.uniform_diffusion_scalar : 0.0;
			const size_t lds = shape.bytes;
			for (int c0 = 0; c0 < e->nt; c0 += 3) {
				const int ntr = std::min(3, e->nt - c0);
#define LAUNCH_SLIDE(N_) do { if (p.closed) hipLaunchKernelGGL((k_v_tracers_explicit_slide<N_, true>), grd, blk, lds, e->stream, p, c0, xin, xup, dt, ks_, (const double *)e->d_ref, nt_, xm, nseg); \
				else hipLaunchKernelGGL((k_v_tracers_explicit_slide<N_, false>), grd, blk, lds, e->stream, p, c0, xin, xup, dt, ks_, (const double *)e->d_ref, nt_, xm, nseg); } while (0)
				if (ntr == 3) LAUNCH_SLIDE(3); else if (ntr == 2) LAUNCH_SLIDE(2); else LAUNCH_SLIDE(1);
#undef LAUNCH_SLIDE
			}
		}
#if TMX_EXP
		else if (e->opt_vt_walk == 4 || e->opt_vt_walk == 5 || e->opt_vt_walk == 6 || e->opt_vt_walk == 8 || e->opt_vt_walk == 10) {      // by column segments of that many levels
			const int nt_ = NTILES(e, p), xm = e->xcd_vertical, kc = e->opt_vt_walk;
			dim3 blk(64), grd(xcd_column_grid(xm, nt_, (p.L + kc - 1) / kc));
#define LAUNCH_WALK(KC_) hipLaunchKernelGGL(k_v_tracers_explicit_walk<KC_>, grd, blk, 0, e->stream, p, e->nt, xin, xup, dt, \
				e->udiff ? e->cfg.uniform_diffusion_scalar : 0.0, (const double *)e->d_ref, nt_, xm)
			if (kc == 4) LAUNCH_WALK(4); else if (kc == 5) LAUNCH_WALK(5); else if (kc == 6) LAUNCH_WALK(6); else if (kc == 8) LAUNCH_WALK(8); else LAUNCH_WALK(10);
#undef LAUNCH_WALK
		}
#endif
		else {
			const int nt_ = NTILES(e, p), xm = e->xcd_vertical;
			dim3 blk(64, 8), grd(xcd_column_grid(xm, nt_, (p.L + 7) / 8));
			hipLaunchKernelGGL(k_v_tracers_explicit_tile, grd, blk, 0, e->stream, p, e->nt, xin, xup, dt,
				e->udiff ? e->cfg.uniform_diffusion_scalar : 0.0, (const double *)e->d_ref, nt_, xm);
		}
		return 0;
	}
	return launch_vt_explicit_column(e, p, xin, xup, dt);
}

__global__ __launch_bounds__(256) void k_v_filter_tracers(KParams p, int nt, const double * __restrict__ area, double * x) {
	const int L = p.L;
	const size_t NS = (size_t)p.NS;
	const int col = blockIdx.x * 256 + threadIdx.x;
	const int c = blockIdx.y;
	if (col >= p.ncol || c >= nt) return;
	double total = 0.0, nonneg = 0.0;
	for (int k = 0; k < L; k++) {
		const double q = x[(size_t)TMX_SLAB_Q(L, c, k) * NS + col];
		const double pm = q * area[(size_t)k * NS + col];
		total += pm;
		if (q >= 0.0) nonneg += pm;
	}
	const double r = total / nonneg;
	for (int k = 0; k < L; k++) {
		const size_t o = (size_t)TMX_SLAB_Q(L, c, k) * NS + col;
		const double q = x[o];
		x[o] = (q > 0.0) ? q * r : 0.0;
	}
}

void tmxk_v_filter_tracers(tmx_engine * e, const KParams & p, double * x) {
	if (e->nt == 0) return;
	hipLaunchKernelGGL(k_v_filter_tracers, dim3((p.ncol + 255) / 256, e->nt), dim3(256), 0, e->stream, p, e->nt, (const double *)e->d_area, x);
}

// ---------------------------------------------------------------------------------------------
// VerticalDynamicsFEM::StepImplicitTermsExplicitly (src/atm/VerticalDynamicsFEM.cpp:439-612):
// update -= dt * F(initial) for rho*theta, W, rho on EVERY column (F = BuildF of the initial column).

// UD (fully explicit mode with uniform diffusion): F additionally holds the vertical diffusion of rho*theta and W
// relative to the reference column xref (cs = K_s / ztop^2, cw = K_v / ztop^2).
// UVX: the thread of (column, level k < L) also applies V.StepExplicit's update of U,V (v_explicit_point: penalty and, with UD,
// the vertical diffusion), which reads the same U,V,W columns and metric rows -- one launch less per stage and the operands
// found in the cache
template <bool UD, bool UVX>
// KT_VC levels per workgroup.  A thread reads the levels k-2 .. k+2 of its column, so the level tiles of a column overlap by
// four levels and every value is fetched 2.7 times over at the L2's memory side (PMC, ne30 L40: 514 MB of reads per launch for
// 190 MB of operands: the level-neighbour tiles are 1 350 workgroups apart in dispatch order, on another XCD's L2).  Taller
// tiles make the neighbours wavefronts of one workgroup, and lose: config 4's step takes 5.12 / 5.21 / 5.34 ms with 4 / 8 / 16
// levels per workgroup (1 024-thread workgroups leave one per CU).  4 stays.
#ifndef KT_VC
#define KT_VC 4
#endif
__global__ __launch_bounds__(64 * KT_VC) void k_vi_terms_explicit(KParams p, const double * __restrict__ xin,
	double * __restrict__ xup, double dt, const double * __restrict__ xref, double cs, double cw, int ntile, int xmode)
{
	const int L = p.L;
	const size_t NS = (size_t)p.NS;
	int bx, by;
	if (!xcd_column_tile(xmode, ntile, (L + 1 + KT_VC - 1) / KT_VC, bx, by)) return;
	const int col = (p.quads ? p.quads[bx] : bx) * 64 + threadIdx.x;
	const int k = by * KT_VC + WAVE_UNIFORM(threadIdx.y);
	if (col >= p.ncol || k > L) return;
	ColConst cc;
	cc.c2a0 = p.g2d[G2_C2A0 * NS + col]; cc.c2a1 = p.g2d[G2_C2A1 * NS + col]; cc.c2b1 = p.g2d[G2_C2B1 * NS + col];
	cc.jn = p.g2d[G2_JN * NS + col]; cc.je = p.g2d[G2_JE * NS + col]; cc.drx = p.g2d[G2_DRX * NS + col];
	cc.invdt = 1.0 / dt; cc.upc = 0.5 * (1.0 / (double)L); cc.cv = p.cp - p.Rd;
	const MetCol mcol = met_col(p, col);
	// the values to update, loaded with the operands (at the point of use their latency would follow the whole evaluation)
	const double upW = xup[TMX_SLAB_W(L, k) * NS + col];
	const double upT = (k < L) ? xup[TMX_SLAB_T(L, k) * NS + col] : 0.0, upR = (k < L) ? xup[TMX_SLAB_R(L, k) * NS + col] : 0.0;
	const NodeLev nA = load_node(p, mcol, xin, k - 1, col), nB = load_node(p, mcol, xin, k, col), nC = load_node(p, mcol, xin, k + 1, col);
	const EdgeLev eA = load_edge(p, mcol, xin, k - 1, col), eB = load_edge(p, mcol, xin, k, col), eC = load_edge(p, mcol, xin, k + 1, col);
	double rP[TMX_BW], rW[TMX_BW], rR[TMX_BW], fP, fW, fR;
	BlkCarry cy;
	double udP = 0.0, udW = 0.0;
	if (UD) {
		// PrepareColumn :2104-2160: DiffDiff of the column minus DiffDiff of the reference column; W not on the boundaries
		if (k < L) {
			double dd = 0.0, ddr = 0.0;
#pragma unroll
			for (int off = -2; off <= 2; off++) {
				const int l = k + off;
				if (l < 0 || l >= L) continue;
				const double c = OPC(TMX_OP_DIFFDIFF_NODE_TO_NODE, k, off);
				dd += c * xin[(size_t)TMX_SLAB_T(L, l) * NS + col];
				ddr += c * xref[(size_t)TMX_SLAB_T(L, l) * NS + col];
			}
			udP = cs * (dd - ddr);
		}
		if (k > 0 && k < L) {
			double dd = 0.0, ddr = 0.0;
#pragma unroll
			for (int off = -2; off <= 2; off++) {
				const int l = k + off;
				if (l < 0 || l > L) continue;
				const double c = OPC(TMX_OP_DIFFDIFF_REDGE_TO_REDGE, k, off);
				dd += c * xin[(size_t)TMX_SLAB_W(L, l) * NS + col];
				ddr += c * xref[(size_t)TMX_SLAB_W(L, l) * NS + col];
			}
			udW = cw * (dd - ddr);
		}
	}
	compute_block<false, UD>(p, p.ops, cc, k, nA, nB, nC, eA, eB, eC, rP, rW, rR, fP, fW, fR, cy, udP, udW);
	if (k < L) {
		xup[TMX_SLAB_T(L, k) * NS + col] = upT - dt * fP;
		xup[TMX_SLAB_R(L, k) * NS + col] = upR - dt * fR;
	}
	xup[TMX_SLAB_W(L, k) * NS + col] = upW - dt * fW;
	if (UVX && k < L) v_explicit_point<UD>(p, xin, xup, dt, xref, cw, col, k);
}

// The same update by a thread that walks a column (or one of `nseg` segments of it) block row by block row, as the column solve's
// assembly does: the three node levels and three interfaces a block row touches in a sliding register window, the quantities a
// block row shares with the next carried over (compute_block<CARRY>: one evaluation of the Exner function per level instead of
// two, every state value loaded once instead of three to five times), the next levels loaded two iterations ahead, operator
// coefficients and the 1 - eta table in LDS.  The uniform-diffusion stencils take the state's five levels from the window (the
// value that has just left it, the three in it, the one about to enter) and keep sliding windows of the reference's.  A segment that
// does not start at the bottom evaluates the block row below it first, only to fill the carry.  Same statements on the same
// operands as k_vi_terms_explicit: bit-identical (tested).
template <bool UD, bool CLOSED>
__global__ __launch_bounds__(128) void k_vi_terms_explicit_slide(KParams p, const double * __restrict__ xin,
	double * __restrict__ xup, double dt, const double * __restrict__ xref, double cs, double cw, int ntile, int xmode, int nseg)
{
	extern __shared__ double opsl_mem[];
	double * opsl = opsl_mem;
	const int L = p.L;
	constexpr int MM = CLOSED ? 1 : 2;
	double * etal = opsl_mem + TMX_OP_COUNT * (L + 1) * TMX_OPW;
	// the exp / log tables of the Exner function in LDS too: read from global memory each lookup is a vector-memory load behind an
	// s_waitcnt vmcnt(0), i.e. two waits per block row for every level prefetch in flight (the column solve's assembly: the same)
	double * rmtab = etal + 2 * L + 1;
	walk_tables_to_lds<CLOSED>(p, opsl, etal);
	tmx_rm_tables_to_lds(rmtab, threadIdx.y * 64 + threadIdx.x, 128);
	__syncthreads();
	const size_t NS = (size_t)p.NS;
	int col, k0, k1;      // block rows k0 .. k1 - 1 of 0 .. L
	if (!walk_segment(p, xmode, ntile, nseg, L + 1, col, k0, k1)) return;
	ColConst cc;
	cc.c2a0 = p.g2d[G2_C2A0 * NS + col]; cc.c2a1 = p.g2d[G2_C2A1 * NS + col]; cc.c2b1 = p.g2d[G2_C2B1 * NS + col];
	cc.jn = p.g2d[G2_JN * NS + col]; cc.je = p.g2d[G2_JE * NS + col]; cc.drx = p.g2d[G2_DRX * NS + col];
	cc.invdt = 1.0 / dt; cc.upc = 0.5 * (1.0 / (double)L); cc.cv = p.cp - p.Rd;
	const MetCol mcol = met_col(p, col);
	const int kw = (k0 > 0) ? k0 - 1 : 0;      // first block row evaluated (k0 - 1: for the carry only)
	// The window: block row k reads U, V, rho*theta, rho of the levels k - 1, k, k + 1 and W of the interfaces k - 1, k, k + 1; with the
	// carry, the metric terms of level k and of the interfaces k, k + 1 only.  Levels k + 2 and k + 3 are in flight as raw values
	// (their metric terms are arithmetic on per-column factors and the LDS table: evaluated when a level becomes the window's top).
	struct Raw { double un, vn, pn, rn, we; };
	auto raw = [&](int l) {      // (out-of-range levels carry the values of the nearest one, as load_node / load_edge)
		Raw r;
		const int lc = l < 0 ? 0 : (l >= L ? L - 1 : l), le = l < 0 ? 0 : (l > L ? L : l);
		r.un = xin[TMX_SLAB_U(L, lc) * NS + col]; r.vn = xin[TMX_SLAB_V(L, lc) * NS + col];
		r.pn = xin[TMX_SLAB_T(L, lc) * NS + col]; r.rn = xin[TMX_SLAB_R(L, lc) * NS + col];
		r.we = xin[TMX_SLAB_W(L, le) * NS + col];
		return r;
	};
	auto node_of = [&](const Raw & r, int l) {
		NodeLev n; n.un = r.un; n.vn = r.vn; n.pn = r.pn; n.rn = r.rn;
		const int lc = l < 0 ? 0 : (l >= L ? L - 1 : l);
		metric_node3<MM>(p, mcol, lc, col, n.ca2, n.cb2, n.cx2, etal);
		return n;
	};
	auto edge_of = [&](const Raw & r, int l) {
		EdgeLev e; e.we = r.we;
		const int le = l < 0 ? 0 : (l > L ? L : l);
		metric_edge<MM>(p, mcol, le, col, e.ce0, e.ce1, e.ce2, etal);
		return e;
	};
	Raw rA = raw(kw - 1), rN = raw(kw + 2);
	NodeLev nB = load_node<MM>(p, mcol, xin, kw, col, etal), nC = load_node<MM>(p, mcol, xin, kw + 1, col, etal);
	EdgeLev eB = load_edge<MM>(p, mcol, xin, kw, col, etal), eC = load_edge<MM>(p, mcol, xin, kw + 1, col, etal);
	double pm2 = 0.0, wm2 = 0.0;      // rho*theta of level k - 2, W of interface k - 2 (what has left the window)
	double tr[5] = { 0, 0, 0, 0, 0 }, wr[5] = { 0, 0, 0, 0, 0 };      // reference rho*theta on the levels, W on the interfaces k - 2 .. k + 2
	auto ref_T = [&](int l) { return (UD && l >= 0 && l < L) ? xref[(size_t)TMX_SLAB_T(L, l) * NS + col] : 0.0; };
	auto ref_W = [&](int l) { return (UD && l >= 0 && l <= L) ? xref[(size_t)TMX_SLAB_W(L, l) * NS + col] : 0.0; };
	if (UD) {
		if (kw - 2 >= 0) { pm2 = xin[(size_t)TMX_SLAB_T(L, kw - 2) * NS + col]; wm2 = xin[(size_t)TMX_SLAB_W(L, kw - 2) * NS + col]; }
#pragma unroll
		for (int t = 0; t < 5; t++) { tr[t] = ref_T(kw - 2 + t); wr[t] = ref_W(kw - 2 + t); }
	}
	double upT = 0.0, upR = 0.0, upW = 0.0;
	if (kw == k0) {
		upW = xup[TMX_SLAB_W(L, kw) * NS + col];
		if (kw < L) { upT = xup[TMX_SLAB_T(L, kw) * NS + col]; upR = xup[TMX_SLAB_R(L, kw) * NS + col]; }
	}
	BlkCarry cy = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll 1
	for (int k = kw; k < k1; k++) {
		// two levels ahead: the level that enters the window after the next block row; the reference's entering values and the
		// values the next block row updates
		const Raw rNN = raw(k + 3);
		const double trn = ref_T(k + 3), wrn = ref_W(k + 3);
		double upTn = 0.0, upRn = 0.0, upWn = 0.0;
		if (k + 1 < k1) {
			upWn = xup[TMX_SLAB_W(L, k + 1) * NS + col];
			if (k + 1 < L) { upTn = xup[TMX_SLAB_T(L, k + 1) * NS + col]; upRn = xup[TMX_SLAB_R(L, k + 1) * NS + col]; }
		}
		double udP = 0.0, udW = 0.0;
		if (UD) {
			const double tw[5] = { pm2, rA.pn, nB.pn, nC.pn, rN.pn }, ww[5] = { wm2, rA.we, eB.we, eC.we, rN.we };
			if (k < L) {
				double dd = 0.0, ddr = 0.0;
#pragma unroll
				for (int off = -2; off <= 2; off++) {
					const int l = k + off;
					if (l < 0 || l >= L) continue;
					const double c = OPCL(TMX_OP_DIFFDIFF_NODE_TO_NODE, k, off);
					dd += c * tw[off + 2];
					ddr += c * tr[off + 2];
				}
				udP = cs * (dd - ddr);
			}
			if (k > 0 && k < L) {
				double dd = 0.0, ddr = 0.0;
#pragma unroll
				for (int off = -2; off <= 2; off++) {
					const int l = k + off;
					if (l < 0 || l > L) continue;
					const double c = OPCL(TMX_OP_DIFFDIFF_REDGE_TO_REDGE, k, off);
					dd += c * ww[off + 2];
					ddr += c * wr[off + 2];
				}
				udW = cw * (dd - ddr);
			}
		}
		double rP[TMX_BW], rW[TMX_BW], rR[TMX_BW], fP, fW, fR;
		{
			NodeLev nA; nA.un = rA.un; nA.vn = rA.vn; nA.pn = rA.pn; nA.rn = rA.rn; nA.ca2 = 0.0; nA.cb2 = 0.0; nA.cx2 = 0.0;      // (with the carry a block row reads no metric term of level k - 1)
			EdgeLev eA; eA.we = rA.we; eA.ce0 = 0.0; eA.ce1 = 0.0; eA.ce2 = 0.0;
			compute_block<true, UD>(p, opsl, cc, k, nA, nB, nC, eA, eB, eC, rP, rW, rR, fP, fW, fR, cy, udP, udW, rmtab);
		}
		const double resT = upT - dt * fP, resR = upR - dt * fR, resW = upW - dt * fW;
		pm2 = rA.pn; wm2 = rA.we;
		rA.un = nB.un; rA.vn = nB.vn; rA.pn = nB.pn; rA.rn = nB.rn; rA.we = eB.we;
		nB = nC; eB = eC;
		nC = node_of(rN, k + 2); eC = edge_of(rN, k + 2);
		rN = rNN;
		tr[0] = tr[1]; tr[1] = tr[2]; tr[2] = tr[3]; tr[3] = tr[4]; tr[4] = trn;
		wr[0] = wr[1]; wr[1] = wr[2]; wr[2] = wr[3]; wr[3] = wr[4]; wr[4] = wrn;
		upT = upTn; upR = upRn; upW = upWn;
		// The block row's stores LAST, behind the window's move (which evaluates the metric terms of the level that enters, i.e. reads values
		// loaded an iteration ago): the stores sit in a branch, the compiler cannot count them, and a loaded value first used behind them waits
		// for everything in flight -- the stores' own completion and the prefetch of two levels ahead -- once per block row.  The values the
		// next block row updates are made to land before the stores too (they were loaded with this block row's operands).
		asm volatile("" : "+v"(upT), "+v"(upR), "+v"(upW));
		if (k >= k0) {
			if (k < L) {
				xup[TMX_SLAB_T(L, k) * NS + col] = resT;
				xup[TMX_SLAB_R(L, k) * NS + col] = resR;
			}
			xup[TMX_SLAB_W(L, k) * NS + col] = resW;
		}
	}
}

void tmxk_vi_terms_explicit(tmx_engine * e, const KParams & p, const double * xin, double * xup, double dt, bool with_uv) {
	const int nt_ = NTILES(e, p), xm = e->xcd_vertical;
	const WalkShape shape = vwalk_shape(TMX_WALK_VITE, p.L, e->opt_vite_walk, nt_, with_uv);
	e->vwalk_launched[TMX_WALK_VITE] = shape.nseg;      // (tmx_info(TMX_INFO_VERTICAL_KERNELS): the walk's segments, 0 the level-parallel kernel below)
	if (shape.nseg) {      // a thread walks (a segment of) its column; -n = n segments, -1000 = chosen from the grid size
		const int nseg = shape.nseg;
		const size_t lds_slide = shape.bytes;
		dim3 blk(64, 2), grd(xcd_column_grid(xm, nt_, (nseg + 1) / 2));
		const bool ud = e->udiff && e->fully_explicit;
		const double z2 = e->cfg.ztop * e->cfg.ztop;
		const double cs = ud ? e->cfg.uniform_diffusion_scalar / z2 : 0.0, cw = ud ? e->cfg.uniform_diffusion_vector / z2 : 0.0;
#define LAUNCH_VS(UD_, CL_) hipLaunchKernelGGL((k_vi_terms_explicit_slide<UD_, CL_>), grd, blk, lds_slide, e->stream, p, xin, xup, dt, (const double *)(ud ? e->d_ref : nullptr), cs, cw, nt_, xm, nseg)
		if (ud) { if (p.closed) LAUNCH_VS(true, true); else LAUNCH_VS(true, false); }
		else { if (p.closed) LAUNCH_VS(false, true); else LAUNCH_VS(false, false); }
#undef LAUNCH_VS
		return;
	}
	dim3 blk(64, KT_VC), grd(xcd_column_grid(xm, nt_, (p.L + 1 + KT_VC - 1) / KT_VC));
	if (e->udiff && e->fully_explicit) {
		const double z2 = e->cfg.ztop * e->cfg.ztop;
#if TMX_EXP      // (option "vx_fused", measured slower: experiments flavour only)
		if (with_uv) hipLaunchKernelGGL((k_vi_terms_explicit<true, true>), grd, blk, 0, e->stream, p, xin, xup, dt, (const double *)e->d_ref,
			e->cfg.uniform_diffusion_scalar / z2, e->cfg.uniform_diffusion_vector / z2, nt_, xm);
		else
#endif
		hipLaunchKernelGGL((k_vi_terms_explicit<true, false>), grd, blk, 0, e->stream, p, xin, xup, dt, (const double *)e->d_ref,
			e->cfg.uniform_diffusion_scalar / z2, e->cfg.uniform_diffusion_vector / z2, nt_, xm);
	} else
		hipLaunchKernelGGL((k_vi_terms_explicit<false, false>), grd, blk, 0, e->stream, p, xin, xup, dt, (const double *)nullptr, 0.0, 0.0, nt_, xm);
}
