// tmx_device.h -- device-side helpers shared by the kernel translation units (tmx_k_*.hip): addressing, stage combinations,
// XCD-aware tile orders, the terrain-following metric, the Exner function.  gfx950 only.
#pragma once
#include "tmx_internal.h"
#include "tmx_refmath.h"

#ifndef KT_H
#define KT_H 4      // levels per workgroup of the horizontal kernels (256 threads); 2 / 3 measure the same, 5 / 6 / 8: explicit stage 0.77 / 0.75 / 0.69 against 0.56 ms per step
                    // (three resident wavefronts per SIMD hold whole 4-wavefront workgroups only; taller tiles leave slots empty)
#endif

// Update statement a - l*u of the band LU (dgbtf2's rank-1 update, dgbtrs' forward sweep, dtbsv's column sweep).
// LAPACK builds them from dger / dtbsv, and the optimised BLAS libraries the reference links (MKL, OpenBLAS) evaluate
// those with fused multiply-adds: the reference linked against either agrees BIT FOR BIT, and the C oracle reproduces
// its implicit step bit for bit only with the update fused (tests/golden/lapack_spread.json,
// test_percall_chain).  So the fused form IS the reference's arithmetic; everything else in this file stays unfused
// (-ffp-contract=off), as the reference's own C++ is compiled without FMA contraction.
// The band LU's updates a - l * u: fused multiply-adds, as OpenBLAS's and MKL's kernels evaluate them on x86-64-v3 hosts
// (DESIGN.md section 2).  A reference linked to a BLAS WITHOUT fused multiply-adds (a plain netlib build, MKL on some AMD
// hosts) is reproduced by multiply and subtract, rounded separately (-ffp-contract=off): the translation units whose kernels use
// LU_UPD (the Makefile's SRC_LU: tmx_k_column.hip, tmx_k_tracer_solve.hip) are compiled a second time with -DTMX_LU_NOFMA into
// the same library, and the engine's option "lu_fma" = 0 (TMX_LU_FMA=0) selects that pass at run time (tmx_lu_select.hip).
#ifdef TMX_LU_NOFMA
#define LU_UPD(a, l, u) ((a) - (l) * (u))
#else
#define LU_UPD(a, l, u) __builtin_fma(-(l), (u), (a))
#endif

#define OPC(op, k, off) p.ops[(((op) * (p.L + 1)) + (k)) * TMX_OPW + ((off) + 2)]

// Linear combination of state instances in the reference's accumulation order
// (GridPatch::LinearCombineData, src/atm/GridPatch.cpp:1436-1508): v = c_d * X_d (or 0), then += c_m * X_m.
// dmask (node-unique kernels instantiated with DM only): bit m set = term m is an ELEMENT-MAJOR instance whose copies of a node may differ
// (the model state behind a per-copy operation such as the Held-Suarez forcing): the thread reads its own copy, slab stride NS, the
// thread's own column; bit 31: the same for the stage's initial instance.  The kernels' results are node-unique either way.
struct LinTerms { const double * src[12]; double coef[12]; int n; int premul; unsigned dmask; };
// Where the U,V slabs of the instances named by a LinTerms (and of the stage's initial instance) live: the instance's own slot,
// or the slot of the instance it was copied from when the stepper left the CopyData of U,V out (tmx_step.hip: the implicit
// column solve rewrites rho*theta, W, rho of the copy but leaves U,V identical to the source's)
struct UvTerms { const double * src[12]; const double * xin; };

// base value of the update instance at flat offset o: either a plain instance (n == 0: src[0] is the base
// pointer) or the linear combination evaluated on the fly, so that LinearCombineData + StepExplicit is one
// pass instead of write + re-read of the combined state.  Same operations in the same order.
// NT = number of entries (compile time, so that every load of the combination is issued at once; a
// run-time loop over the kernel-argument arrays serialises one memory round trip per term).
// Every kernel here is launched with blockDim.x == 64: one wavefront per threadIdx.y.  Telling the compiler
// that the level index is wave-uniform moves the operator coefficients, the 1 - eta table and all slab
// offsets to scalar loads / SALU and frees the vector registers they occupied.
#define WAVE_UNIFORM(v) __builtin_amdgcn_readfirstlane((int)(v))
// 64-column tile of a workgroup: all tiles of the rank's patches, or the entries of a tile list (KParams.quads: the early /
// late tiles of the boundary-first stages); NTILES is the matching grid size on the host
#define TILE_X(p) ((p).quads ? (p).quads[blockIdx.x] : (int)blockIdx.x)
#define NTILES(e, p) ((p).quads ? (e)->launch_tiles : (p).NS / 64)

// Addressing: every global access here is  base pointer + (wave-uniform slab offset) + (lane's column).  Written
// as (uniform 64-bit pointer) + (32-bit per-lane BYTE offset) it maps onto the saddr form of global_load /
// global_store -- one 32-bit VGPR offset shared by all accesses of a thread instead of a 64-bit VGPR address
// (2 registers + a v_lshl_add_u64) per access.  An instance is 104 MB at ne30 L30; a slab row (NS columns) must
// stay below 4 GiB of bytes, checked at finalize.
__device__ __forceinline__ double ldu(const double * uniform_base, unsigned lane_byte_off) {
	return *(const double *)((const char *)uniform_base + lane_byte_off);
}
__device__ __forceinline__ void stu(double * uniform_base, unsigned lane_byte_off, double v) {
	*(double *)((char *)uniform_base + lane_byte_off) = v;
}

// The same in two phases, for kernels that name several slabs of the combination: lin_load issues the loads of one slab's raw
// terms (no control flow: PM = "the destination's own coefficient is not zero" is a compile-time parameter, so the loads of all
// slabs can be issued back to back), lin_reduce combines them in the reference's order.  With base_value_u called slab after
// slab the compiler serialised load batch -> wait -> reduce per slab behind the run-time `premul` branches: five dependent
// memory round trips at the head of every wavefront of the explicit kernels.
template <int NT, bool PM>
__device__ __forceinline__ void lin_load(const double * const (&src)[12], size_t slab_off, unsigned colb, double (&x)[NT > 0 ? NT : 1]) {
	if (NT == 0) { x[0] = ldu(src[0] + slab_off, colb); return; }
#pragma unroll
	for (int m = 0; m < NT; m++) x[m] = (m > 0 || PM) ? ldu(src[m] + slab_off, colb) : 0.0;
}
template <int NT, bool PM>
__device__ __forceinline__ double lin_reduce(const LinTerms & t, const double (&x)[NT > 0 ? NT : 1]) {
	if (NT == 0) return x[0];
	double v = PM ? x[0] * t.coef[0] : 0.0;
#pragma unroll
	for (int m = 1; m < NT; m++) v += t.coef[m] * x[m];
	return v;
}

// Prefix of a LATER stage's combination, formed from the terms this stage has loaded anyway.  The reference accumulates a
// combination in a fixed order -- the destination's own term first, then the other instances in ascending order
// (GridPatch::LinearCombineData) -- so the value after the first k terms is a well-defined intermediate; when the instances of
// those k terms are exactly the instances this stage combines, it can be formed here (same operands, same order, the later
// stage's coefficients) and stored, and the later stage starts from it (coefficient 1: exact) and reads k - 1 instances less.
// ARS343: the third stage combines instances 0..4, the fourth 1, 0, 2, 3, 4, 5, 6: seven source instances become three.
// coef[m] belongs to this stage's term m >= 1; first = this stage's term index of the later stage's destination (-1: it has none).
template <int NT>
__device__ __forceinline__ double emit_value(const EmitTerms & em, const double (&x)[NT > 0 ? NT : 1]) {
	double p = 0.0;
#pragma unroll
	for (int m = 1; m < NT; m++) if (em.first == m) p = x[m] * em.coef[m];
#pragma unroll
	for (int m = 1; m < NT; m++) { const double q = p + em.coef[m] * x[m]; p = (em.first == m) ? p : q; }
	return p;
}
// base_value_u / base_value_uv that also return that prefix (EM: compile-time switch)
template <int NT, bool EM>
__device__ __forceinline__ double base_value_u2(const LinTerms & t, const double * const (&src)[12], const EmitTerms & em, size_t slab_off, unsigned colb, double & pfx) {
	if (NT == 0) return ldu(src[0] + slab_off, colb);
	double x[NT > 0 ? NT : 1];
#pragma unroll
	for (int m = 0; m < NT; m++) x[m] = (m > 0 || t.premul) ? ldu(src[m] + slab_off, colb) : 0.0;
	double v = t.premul ? x[0] * t.coef[0] : 0.0;
#pragma unroll
	for (int m = 1; m < NT; m++) v += t.coef[m] * x[m];
	if (EM) pfx = emit_value<NT>(em, x);
	return v;
}

// base_value with the slab offset (uniform, in doubles) and the lane's byte offset kept apart
template <int NT>
__device__ __forceinline__ double base_value_u(const LinTerms & t, size_t slab_off, unsigned colb) {
	if (NT == 0) return ldu(t.src[0] + slab_off, colb);
	double x[NT > 0 ? NT : 1];
#pragma unroll
	for (int m = 0; m < NT; m++) x[m] = (m > 0 || t.premul) ? ldu(t.src[m] + slab_off, colb) : 0.0;
	double v = t.premul ? x[0] * t.coef[0] : 0.0;
#pragma unroll
	for (int m = 1; m < NT; m++) v += t.coef[m] * x[m];
	return v;
}

// the same for a U or V slab: sources from the UvTerms
template <int NT>
__device__ __forceinline__ double base_value_uv(const LinTerms & t, const UvTerms & uv, size_t slab_off, unsigned colb) {
	if (NT == 0) return ldu(uv.src[0] + slab_off, colb);
	double x[NT > 0 ? NT : 1];
#pragma unroll
	for (int m = 0; m < NT; m++) x[m] = (m > 0 || t.premul) ? ldu(uv.src[m] + slab_off, colb) : 0.0;
	double v = t.premul ? x[0] * t.coef[0] : 0.0;
#pragma unroll
	for (int m = 1; m < NT; m++) v += t.coef[m] * x[m];
	return v;
}

// base_value_u / base_value_uv where some terms are element-major instances (LinTerms::dmask): slab index given, stride and lane offset per term
template <int NT>
__device__ __forceinline__ double base_value_dm(const LinTerms & t, const double * const (&src)[12], int slab, size_t SS, size_t NS, unsigned cb, unsigned gb) {
	auto ld = [&](int m) -> double { const bool d = (t.dmask >> m) & 1u; return ldu(src[m] + (size_t)slab * (d ? NS : SS), d ? gb : cb); };
	if (NT == 0) return ld(0);
	double x[NT > 0 ? NT : 1];
#pragma unroll
	for (int m = 0; m < NT; m++) x[m] = (m > 0 || t.premul) ? ld(m) : 0.0;
	double v = t.premul ? x[0] * t.coef[0] : 0.0;
#pragma unroll
	for (int m = 1; m < NT; m++) v += t.coef[m] * x[m];
	return v;
}

template <int NT>
__device__ __forceinline__ double base_value(const LinTerms & t, size_t o) {
	if (NT == 0) return t.src[0][o];
	double x[NT > 0 ? NT : 1];
#pragma unroll
	for (int m = 0; m < NT; m++) x[m] = (m > 0 || t.premul) ? t.src[m][o] : 0.0;
	double v = t.premul ? x[0] * t.coef[0] : 0.0;
#pragma unroll
	for (int m = 1; m < NT; m++) v += t.coef[m] * x[m];
	return v;
}

// XCD-aware tile order for the gather-heavy DSS kernel.  Workgroups are dealt round-robin over the 8 XCDs
// (b and b+8 share one, each XCD has its own L2), so a 1-D launch is unfolded such that every XCD sweeps a
// contiguous range of group tiles: the 128-byte element rows a tile touches are shared with its
// neighbouring tiles and now stay in one L2 (measured: k_dss 96 -> 79 us at ne30 L30; the streaming H and
// hyperviscosity kernels did not gain and keep the plain 2-D launch).  Placement only affects speed.
__device__ __forceinline__ bool xcd_tile(int nx, int ny, int & x, int & y) {
	const int b = blockIdx.x;
	const int xcd = b & 7, r = b >> 3;
	const int per = (nx + 7) >> 3;            // column tiles per XCD
	y = r / per;                              // level-major inside the XCD
	x = xcd * per + r % per;
	return y < ny && x < nx;
}

// The same for the vertical stencil kernels of the fully explicit mode (explicitly treated terms, U,V penalty, tracer columns):
// a thread of level k reads the levels k - 2 .. k + 2 of its column, so the level blocks of one 64-column tile share most of
// their operands.  In the plain 2-D launch they are a whole row of tiles apart in dispatch order and land on different XCDs
// (the halo levels were fetched 2.7 times over, PMC); here the 1-D launch is unfolded so that the level blocks of a column
// tile are consecutive workgroups of ONE XCD and find the halo in its L2.  mode 0: the plain order (TMX_XCD_VERTICAL=0, A/B).
__device__ __forceinline__ bool xcd_column_tile(int mode, int nx, int ny, int & x, int & y) {
	const int b = blockIdx.x;
	if (!mode) { x = b % nx; y = b / nx; return y < ny; }
	const int xcd = b & 7, r = b >> 3;
	y = r % ny;
	x = (r / ny) * 8 + xcd;
	return x < nx;
}
static inline int xcd_column_grid(int mode, int nx, int ny) { return mode ? ((nx + 7) / 8) * 8 * ny : nx * ny; }

// 3-D terrain-following metric (GridPatchCSGLL.cpp:441-566).  Stored mode streams the reference's arrays;
// closed mode evaluates the same expressions, operation for operation, from eight per-column factors and the
// 1 - eta table (accepted by tmx_set_patch_metric_factors only after a bit-for-bit comparison), which removes
// 8 doubles per point from the explicit kernels' HBM traffic and 6 from the column solve's.
struct MetCol { double mp, ma, mb, mc, daz, dbz, idx, idx2; };
__device__ __forceinline__ MetCol met_col(const KParams & p, int col) {
	MetCol m = { 0, 0, 0, 0, 0, 0, 0, 0 };
	if (p.closed) {
		const size_t NS = (size_t)p.NS;
		m.mp = p.g2d[G2_MP * NS + col]; m.ma = p.g2d[G2_MA * NS + col]; m.mb = p.g2d[G2_MB * NS + col]; m.mc = p.g2d[G2_MC * NS + col];
		m.daz = p.g2d[G2_DAZ * NS + col]; m.dbz = p.g2d[G2_DBZ * NS + col]; m.idx = p.g2d[G2_IDX * NS + col]; m.idx2 = p.g2d[G2_IDX2 * NS + col];
	}
	return m;
}
__device__ __forceinline__ void met_eval(const MetCol & m, double e, double & c0, double & c1, double & c2, double & dra, double & drb) {
	dra = e * m.daz; drb = e * m.dbz;
	c0 = m.mp * (m.ma * dra + m.mb * drb);
	c1 = m.mp * (m.mb * dra + m.mc * drb);
	c2 = m.idx2 - m.idx * (c0 * dra + c1 * drb);
}
// node level k: g^{alpha xi}, g^{beta xi}, g^{xi xi}, d_alpha R, d_beta R
__device__ __forceinline__ void metric_node(const KParams & p, const MetCol & m, int k, int col,
	double & ca2, double & cb2, double & cx2, double & dra, double & drb) {
	if (p.closed) { met_eval(m, p.eta[k], ca2, cb2, cx2, dra, drb); return; }
	const size_t s3 = (size_t)p.L * p.NS, o = (size_t)k * p.NS + col;
	ca2 = p.g3n[G3N_CA2 * s3 + o]; cb2 = p.g3n[G3N_CB2 * s3 + o]; cx2 = p.g3n[G3N_CX2 * s3 + o];
	dra = p.g3n[G3N_DRA * s3 + o]; drb = p.g3n[G3N_DRB * s3 + o];
}
// MM: 0 = metric mode read from p.closed at run time, 1 - eta table in global memory (the explicit kernels);
//     1 = closed form, table in LDS (`etal`); 2 = stored arrays.  1 and 2 are k_vi_fused's compile-time variants:
//     a fixed number of loads per block row lets the compiler count vmcnt exactly, and a pointer that may be LDS
//     or global would become a flat load, which also counts on vmcnt.
template <int MM = 0>
__device__ __forceinline__ void metric_node3(const KParams & p, const MetCol & m, int k, int col, double & ca2, double & cb2, double & cx2,
	const double * etal = nullptr) {
	if (MM == 1 || (MM == 0 && p.closed)) { double a, b; met_eval(m, MM == 1 ? etal[k] : p.eta[k], ca2, cb2, cx2, a, b); return; }
	const size_t s3 = (size_t)p.L * p.NS, o = (size_t)k * p.NS + col;
	ca2 = p.g3n[G3N_CA2 * s3 + o]; cb2 = p.g3n[G3N_CB2 * s3 + o]; cx2 = p.g3n[G3N_CX2 * s3 + o];
}
// interface k: g^{xi alpha}, g^{xi beta}, g^{xi xi}
template <int MM = 0>
__device__ __forceinline__ void metric_edge(const KParams & p, const MetCol & m, int k, int col, double & cx0, double & cx1, double & cx2,
	const double * etal = nullptr) {
	if (MM == 1 || (MM == 0 && p.closed)) { double a, b; met_eval(m, MM == 1 ? etal[p.L + k] : p.eta[p.L + k], cx0, cx1, cx2, a, b); return; }
	const size_t s3 = (size_t)(p.L + 1) * p.NS, o = (size_t)k * p.NS + col;
	cx0 = p.g3e[G3E_CX0 * s3 + o]; cx1 = p.g3e[G3E_CX1 * s3 + o]; cx2 = p.g3e[G3E_CX2 * s3 + o];
}

__device__ __forceinline__ double exner_from_rhotheta(const KParams & p, double rt) {
	// PhysicalConstants::ExnerPressureFromRhoTheta (src/atm/PhysicalConstants.h:397-399)
	return p.cp * tmx_ref_exp(p.Rd / (p.cp - p.Rd) * tmx_ref_log(p.Rd / p.p0 * rt));      // glibc's exp / log, bit for bit (tmx_refmath.h)
}
// The same with the two lookup tables of exp / log in LDS (`rmtab`: 256 doubles {1/c, log c} of log, then the 256 words of
// exp; tmx_rm_tables_to_lds fills it).  From global memory the two dependent table gathers of every evaluation are
// vector-memory loads: in the column kernels each one cost an s_waitcnt vmcnt(0), i.e. a wait for the level prefetches
// (and U-row stores) in flight as well.
// (TMX_RMTAB_DOUBLES = 512: tmx_internal.h, beside the launchers' LDS sizes)
__device__ __forceinline__ void tmx_rm_tables_to_lds(double * rmtab, int tid, int nthreads) {
	for (int t = tid; t < 256; t += nthreads) {
		rmtab[t] = tmx_rm_log_tab[t];
		((unsigned long long *)(rmtab + 256))[t] = tmx_rm_exp_tab[t];
	}
}
// Branch-free form for arguments in the main range of log (positive, normal, finite; the caller checks all lanes with
// exner_arg_in_main_range first): both branches of log are evaluated and selected, exp needs none for these arguments
// (|x| < 2^-54 gives 1.0 on its main path as well).  Same values as exner_from_rhotheta_lds there.
__device__ __forceinline__ bool exner_arg_in_main_range(const KParams & p, double rt) {
	const unsigned top = (unsigned)(tmx_rm_bits(p.Rd / p.p0 * rt) >> 48);
	return top - 0x0010u < 0x7ff0u - 0x0010u;
}
__device__ __forceinline__ double exner_from_rhotheta_bf(const KParams & p, double rt, const double * rmtab) {
	return p.cp * tmx_ref_exp_main(p.Rd / (p.cp - p.Rd) * tmx_ref_log_bf(p.Rd / p.p0 * rt, rmtab), (const unsigned long long *)(rmtab + 256));
}
__device__ __forceinline__ double exner_from_rhotheta_lds(const KParams & p, double rt, const double * rmtab) {
	return p.cp * tmx_ref_exp_t(p.Rd / (p.cp - p.Rd) * tmx_ref_log_t(p.Rd / p.p0 * rt, rmtab), (const unsigned long long *)(rmtab + 256));
}


// DSS combination shared by k_dss (tmx_k_exchange.hip) and the kernels that average while loading (tmx_k_horizontal.hip)
// member M's combination of the copies w0..w3 (values already in M's frame); ty = M's 2-bit pairing type
template <int M>
__device__ __forceinline__ double dss_combine(double w0, double w1, double w2, double w3, int n, int ty) {
	if (n == 2) return 0.5 * (w0 + w1);
	if (n == 4) {
		const double p0 = (ty == 0) ? w0 + w1 : ((ty == 1) ? w0 + w2 : w0 + w3);
		const double p1 = (ty == 0) ? w2 + w3 : ((ty == 1) ? w1 + w3 : w1 + w2);
		return 0.5 * (0.5 * p0 + 0.5 * p1);
	}
	// cube corner: (1/3) * ((x + first) + second), first = next member (ty 0) or previous member (ty 1)
	const double me = (M == 0) ? w0 : ((M == 1) ? w1 : w2);
	const double nx = (M == 0) ? w1 : ((M == 1) ? w2 : w0);
	const double pv = (M == 0) ? w2 : ((M == 1) ? w0 : w1);
	return (1.0 / 3.0) * ((me + (ty ? pv : nx)) + (ty ? nx : pv));
}


// Coefficient (row k, offset off) of operator `op` in a copy of the operator tables: p.ops in global memory (OPC) or staged in LDS (OPCL)
__device__ __forceinline__ double op_coef(const double * ops, int L, int op, int k, int off) { return ops[((op * (L + 1)) + k) * TMX_OPW + (off + 2)]; }
#define OPCL(op, k, off) opsl[(((op) * (p.L + 1)) + (k)) * TMX_OPW + ((off) + 2)]

// The four-node stencil row of an operator that takes node values to interface m (InterpolateNodeToREdge, DifferentiateNodeToREdge:
// LinearColumnOperatorFEM.cpp:1863-1888): nodes m - 2 .. m + 1 in ascending order, the ones outside the column skipped, accumulated
// from 0.0.  val(off) = the value on level m + off, wherever the caller keeps it (a register window: a compile-time index; LDS; global memory).
template <class V>
__device__ __forceinline__ double edge_sum(const double * ops, int L, int op, int m, V val) {
	double s = 0.0;
#pragma unroll
	for (int off = -2; off <= 1; off++) {
		const int l = m + off;
		if (l < 0 || l >= L) continue;
		s += op_coef(ops, L, op, m, off) * val(off);
	}
	return s;
}

// First-order upwind penalty of level k (LinearColumnDiscPenaltyFEM::Apply; VerticalDynamicsFEM.cpp:984-1023, :4153-4181) added to
// `acc`: x(d) = the column's value on level k + d (read only where it exists), w_lo / w_hi = the weights of the interfaces k and k + 1.
// U,V: acc = the value being updated, weights dt |xi_dot|; tracers: acc = 0.0, weights |xi_dot|.
template <class X>
__device__ __forceinline__ double penalty_row(const double * ops, int L, int k, double acc, X x, double w_lo, double w_hi) {
	if (k < L - 1) {
		double b = 0.0;
		b += op_coef(ops, L, TMX_OP_PENALTY_LEFT, k, 0) * x(0);
		b += op_coef(ops, L, TMX_OP_PENALTY_LEFT, k, 1) * x(1);
		acc += b * w_hi;
	}
	if (k > 0) {
		double b = 0.0;
		b += op_coef(ops, L, TMX_OP_PENALTY_RIGHT, k, -1) * x(-1);
		b += op_coef(ops, L, TMX_OP_PENALTY_RIGHT, k, 0) * x(0);
		acc += b * w_lo;
	}
	return acc;
}

// ---------------------------------------------------------------------------------------------
// Element-local operators of ApplyScalarHyperdiffusion / ApplyVectorHyperdiffusion / ComputeCurlAndDiv (HorizontalDynamicsFEM.cpp:1867-2414,
// GridPatchCSGLL.cpp:1132-1305), stated once for the kernels that evaluate them: the hyperviscosity passes (k_hypervis,
// k_hypervis_tracers; k_hypervis_block: the pointwise statements, its contractions stay under its `held` predicate), the uniform diffusion
// (k_uniform_diffusion, k_ref_diffusion_terms) and the tracers' diffusive flux (k_h_tracers<UD>).  k_h_walk<UD> keeps its own copy of
// k_uniform_diffusion's statements and k_hv_walk k_hypervis's: the registers of the one are counted, the other ran 1.5 % longer per launch
// with the shared ones (profiles/viscosity_operators_statement_list.md).
// An element's 16 nodes lie in one run of an LDS row, node (i, j) at eb + 4 i + j.  Where the operands come from, barriers, prefetches and
// stores stay with each kernel.  Operand order as in the reference; nothing is contracted (-ffp-contract=off).
// ElPos: the thread's node (i, j), its element's base offset eb in an LDS row, and the row positions the contractions run over: la[t] = node
// (t, j) along alpha, lb[t] = node (i, t) along beta.  They are formed by the caller (el_pos, from its lane), not inside the contractions:
// there the compiler knows which bits of the lane each term holds and keeps one address per access, as in the hand-written loops; formed
// from i, j, eb inside the contractions, the addresses come out as chains of base + constant (k_hv_walk, when tried: 7 registers, 4 bytes of scratch more).
struct ElPos { int i, j, eb, la[4], lb[4]; };
__device__ __forceinline__ ElPos el_pos(int lane, int eb) {
	ElPos e;
	e.i = (lane & 15) >> 2; e.j = lane & 3; e.eb = eb;
#pragma unroll
	for (int t = 0; t < 4; t++) { e.la[t] = eb + 4 * t + e.j; e.lb[t] = eb + 4 * e.i + t; }
	return e;
}
struct ElPair { double a, b; };

// da[n] = d/dalpha of row ra[n], db[n] = d/dbeta of row rb[n]: contraction with the derivative matrix sD, then the patch's 1 / element spacing
template <int N, int NR, int RL>
__device__ __forceinline__ void el_deriv(double (&s)[NR][RL], const double (&sD)[16], const ElPos & e, const int (&ra)[N], const int (&rb)[N],
	double ida, double idb, double (&da)[N], double (&db)[N])
{
#pragma unroll
	for (int n = 0; n < N; n++) da[n] = db[n] = 0.0;
#pragma unroll
	for (int t = 0; t < 4; t++) {
		const double Da = sD[t * 4 + e.i], Db = sD[t * 4 + e.j];
#pragma unroll
		for (int n = 0; n < N; n++) { da[n] += s[ra[n]][e.la[t]] * Da; db[n] += s[rb[n]][e.lb[t]] * Db; }
	}
#pragma unroll
	for (int n = 0; n < N; n++) { da[n] *= ida; db[n] *= idb; }
}
// Contraction with the stiffness matrix sS: the weak divergence of NP flux pairs (alpha component in row pa[n], beta in pb[n]: its two halves
// in ua[n], ub[n]), the weak gradient of NG scalar rows g[n] (ga[n], gb[n]), and both in one pass
template <int NP, int NR, int RL>
__device__ __forceinline__ void el_wdiv(double (&s)[NR][RL], const double (&sS)[16], const ElPos & e, const int (&pa)[NP], const int (&pb)[NP],
	double ida, double idb, double (&ua)[NP], double (&ub)[NP])
{
#pragma unroll
	for (int n = 0; n < NP; n++) ua[n] = ub[n] = 0.0;
#pragma unroll
	for (int t = 0; t < 4; t++) {
		const double Sa = sS[e.i * 4 + t], Sb = sS[e.j * 4 + t];
#pragma unroll
		for (int n = 0; n < NP; n++) { ua[n] += s[pa[n]][e.la[t]] * Sa; ub[n] += s[pb[n]][e.lb[t]] * Sb; }
	}
#pragma unroll
	for (int n = 0; n < NP; n++) { ua[n] *= ida; ub[n] *= idb; }
}
template <int NG, int NR, int RL>
__device__ __forceinline__ void el_wgrad(double (&s)[NR][RL], const double (&sS)[16], const ElPos & e, const int (&g)[NG], double ida, double idb,
	double (&ga)[NG], double (&gb)[NG])
{
#pragma unroll
	for (int n = 0; n < NG; n++) ga[n] = gb[n] = 0.0;
#pragma unroll
	for (int t = 0; t < 4; t++) {
		const double Sa = sS[e.i * 4 + t], Sb = sS[e.j * 4 + t];
#pragma unroll
		for (int n = 0; n < NG; n++) { ga[n] -= Sa * s[g[n]][e.la[t]]; gb[n] -= Sb * s[g[n]][e.lb[t]]; }
	}
#pragma unroll
	for (int n = 0; n < NG; n++) { ga[n] *= ida; gb[n] *= idb; }
}
template <int NP, int NG, int NR, int RL>
__device__ __forceinline__ void el_stiff(double (&s)[NR][RL], const double (&sS)[16], const ElPos & e, const int (&pa)[NP], const int (&pb)[NP], const int (&g)[NG],
	double ida, double idb, double (&ua)[NP], double (&ub)[NP], double (&ga)[NG], double (&gb)[NG])
{
#pragma unroll
	for (int n = 0; n < NP; n++) ua[n] = ub[n] = 0.0;
#pragma unroll
	for (int n = 0; n < NG; n++) ga[n] = gb[n] = 0.0;
#pragma unroll
	for (int t = 0; t < 4; t++) {
		const double Sa = sS[e.i * 4 + t], Sb = sS[e.j * 4 + t];
#pragma unroll
		for (int n = 0; n < NP; n++) { ua[n] += s[pa[n]][e.la[t]] * Sa; ub[n] += s[pb[n]][e.lb[t]] * Sb; }
#pragma unroll
		for (int n = 0; n < NG; n++) { ga[n] -= Sa * s[g[n]][e.la[t]]; gb[n] -= Sb * s[g[n]][e.lb[t]]; }
	}
#pragma unroll
	for (int n = 0; n < NP; n++) { ua[n] *= ida; ub[n] *= idb; }
#pragma unroll
	for (int n = 0; n < NG; n++) { ga[n] *= ida; gb[n] *= idb; }
}
// The pointwise statements between the passes.  Contravariant components times a Jacobian: of a gradient (the scalar Laplacian's flux), of (U, V)
__device__ __forceinline__ ElPair el_flux(double J, double c2a0, double c2a1, double c2b1, double da, double db) {
	return { J * (c2a0 * da + c2a1 * db), J * (c2a1 * da + c2b1 * db) };
}
// divergence (a) and curl (b) from d_alpha (J u^alpha), d_beta (J u^beta), d_alpha u_beta, d_beta u_alpha
__device__ __forceinline__ ElPair el_div_curl(double dajua, double dbjub, double daub, double dbua, double invJ2) {
	return { (dajua + dbjub) * invJ2, (daub - dbua) * invJ2 };
}
// increments of (U, V) from the weak gradients of the divergence (dad, dbd) and of the curl (dac, dbc)
__device__ __forceinline__ ElPair el_vector_update(double nd, double nv, double j2d, double c2a0, double c2a1, double c2b1, double dad, double dbd, double dac, double dbc) {
	return { nd * dad - nv * j2d * (c2a1 * dac + c2b1 * dbc), nd * dbd + nv * j2d * (c2a0 * dac + c2a1 * dbc) };
}
__device__ __forceinline__ double el_scalar_update(double b, double dt, double invJ, double nu, double ua, double ub) { return b - dt * invJ * nu * (ua + ub); }

// ---------------------------------------------------------------------------------------------
// UpdateColumnTracers (VerticalDynamicsFEM.cpp:3943-4233): the right-hand side of a tracer's column update, stated once for every
// kernel of tmx_k_vertical.hip that evaluates it -- whichever way it spreads the work and wherever it keeps the operands.
// Tracer flux through interface m (:4092-4140): J_e x (tracer density on the interface) x xi_dot, none through the boundaries; with
// uniform diffusion (ud) minus K_s x (rho on the interface) x d/dxi of the mixing ratio's deviation from the reference column's.
// qn(off), mixr(off): tracer density and that deviation on level m + off.
template <class Q, class M>
__device__ __forceinline__ double tracer_edge_flux(const double * ops, int L, int m, double je, double xd, bool ud, double ks, double re, Q qn, M mixr) {
	const double qe = edge_sum(ops, L, TMX_OP_INTERP_NODE_TO_REDGE, m, qn);
	double mf = (m == 0 || m == L) ? 0.0 : je * qe * xd;
	if (ud && m > 0 && m < L) mf -= ks * re * edge_sum(ops, L, TMX_OP_DIFF_NODE_TO_REDGE, m, mixr);
	return mf;
}
// Row k: the divergence of the fluxes through the interfaces k and k + 1 over J_n, minus the upwind penalty `aux` (penalty_row from 0.0)
__device__ __forceinline__ double tracer_rhs_row(const double * ops, int L, int k, double mf_lo, double mf_hi, double jn, double aux) {
	double dmf = 0.0;
	dmf += op_coef(ops, L, TMX_OP_DIFF_REDGE_TO_NODE, k, 0) * mf_lo;
	dmf += op_coef(ops, L, TMX_OP_DIFF_REDGE_TO_NODE, k, 1) * mf_hi;
	double F = dmf / jn;
	F -= aux;
	return F;
}
// Row k for a thread that forms both of its fluxes itself: xdf(m) = xi_dot the flux is taken with, xdp(m) = xi_dot of the initial
// column (the penalty's weight), re(m) = rho on interface m (read under ud only); here qn(l), mixr(l) take the level itself
template <class Q, class M, class XF, class XP, class R>
__device__ __forceinline__ double tracer_rhs_level(const double * ops, int L, int k, double je, double jn, bool ud, double ks, Q qn, M mixr, XF xdf, XP xdp, R re) {
	double mf[2];
#pragma unroll
	for (int mo = 0; mo <= 1; mo++) {
		const int m = k + mo;
		mf[mo] = tracer_edge_flux(ops, L, m, je, xdf(m), ud, ks, ud ? re(m) : 0.0, [&](int off) { return qn(m + off); }, [&](int off) { return mixr(m + off); });
	}
	const double aux = penalty_row(ops, L, k, 0.0, [&](int d) { return qn(k + d); }, fabs(xdp(k)), fabs(xdp(k + 1)));
	return tracer_rhs_row(ops, L, k, mf[0], mf[1], jn, aux);
}
// The fully explicit mode's "solve": the matrix is the diagonal 1/dt, dgbtrs leaves b_j / (1/dt) and skips a zero b_j
__device__ __forceinline__ double tracer_explicit_solve(double F, double idt) {
	if (F != 0.0) F /= idt;
	return F;
}

// ---------------------------------------------------------------------------------------------
// V explicit (implicit mode): xi_dot on interfaces and first-order upwind penalty on U,V
// (src/atm/VerticalDynamicsFEM.cpp:816-828, 984-1023; LinearColumnOperatorFEM.cpp:1863-1888).

__device__ __forceinline__ double xidot_edge(const KParams & p, const double * __restrict__ xin, int kk, int col) {
	const int L = p.L;
	const size_t NS = (size_t)p.NS;
	if (kk <= 0 || kk >= L) return 0.0;
	// U,V on interfaces = InterpolateNodeToREdge of the node values (H prologue, :817-831)
	const double ue = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, kk, [&](int off) { return xin[TMX_SLAB_U(L, kk + off) * NS + col]; });
	const double ve = edge_sum(p.ops, L, TMX_OP_INTERP_NODE_TO_REDGE, kk, [&](int off) { return xin[TMX_SLAB_V(L, kk + off) * NS + col]; });
	const double we = xin[TMX_SLAB_W(L, kk) * NS + col];
	double e0, e1, e2;
	metric_edge(p, met_col(p, col), kk, col, e0, e1, e2);
	return e0 * ue + e1 * ve + e2 * we;
}

// UDV: the vertical uniform diffusion of U,V of the fully explicit mode (k_v_uniform_diffusion_uv below, :1059-1105) is added
// to the same value before it is stored -- the sum the two kernels form through memory, in the same order
#ifndef KT_VE
#define KT_VE 4       // levels per workgroup (vertical stencils: see KT_VC)
#endif
// the update of U,V at (col, level k), k < L
template <bool UDV>
__device__ __forceinline__ void v_explicit_point(const KParams & p, const double * __restrict__ xin, double * __restrict__ xup, double dt,
	const double * __restrict__ xref, double cf, int col, int k)
{
	const int L = p.L;
	const size_t NS = (size_t)p.NS;
	const double up0[2] = { xup[(size_t)k * NS + col], xup[(size_t)(L + k) * NS + col] };      // U, V to update: loaded with the operands
	const double w_hi = dt * fabs(xidot_edge(p, xin, k + 1, col));   // weight of interface k+1
	const double w_lo = dt * fabs(xidot_edge(p, xin, k, col));       // weight of interface k
	const int km = (k > 0) ? k - 1 : 0, kp = (k < L - 1) ? k + 1 : L - 1;
#pragma unroll
	for (int v = 0; v < 2; v++) {
		const int sb = v * L;
		const double x3[3] = { xin[(size_t)(sb + km) * NS + col], xin[(size_t)(sb + k) * NS + col], xin[(size_t)(sb + kp) * NS + col] };
		double out = penalty_row(p.ops, L, k, up0[v], [&](int d) { return x3[d + 1]; }, w_lo, w_hi);
		if (UDV) {
			double dd = 0.0, ddr = 0.0;
#pragma unroll
			for (int off = -2; off <= 2; off++) {
				const int l = k + off;
				if (l < 0 || l >= L) continue;
				const double c = OPC(TMX_OP_DIFFDIFF_NODE_TO_NODE, k, off);
				dd += c * xin[(size_t)(sb + l) * NS + col];
				ddr += c * xref[(size_t)(sb + l) * NS + col];
			}
			out += dt * cf * (dd - ddr);
		}
		xup[(size_t)(sb + k) * NS + col] = out;
	}
}

// ---------------------------------------------------------------------------------------------
// Frame of the kernels in which a thread walks a column, or one of `nseg` segments of it, row by row (k_v_explicit_slide,
// k_v_tracers_explicit_slide, k_vi_terms_explicit_slide): workgroups of 64 columns x 2 segments, operator tables in LDS.
// The operator tables and, CLOSED, the 1 - eta table go to LDS (`opsl`: [TMX_OP_COUNT][L + 1][TMX_OPW], `etal`: [2 L + 1]); the
// caller's barrier follows.  The walks store to the update instance inside their loop, after which the compiler may not read the
// tables through the scalar cache any more (the stores might alias them) -- and as vector loads each one waits for every load in
// flight (s_waitcnt vmcnt(0)), the prefetched level included.
template <bool CLOSED>
__device__ __forceinline__ void walk_tables_to_lds(const KParams & p, double * opsl, double * etal) {
	const int tid = threadIdx.y * 64 + threadIdx.x;
	for (int t = tid; t < TMX_OP_COUNT * (p.L + 1) * TMX_OPW; t += 128) opsl[t] = p.ops[t];
	if (CLOSED) for (int t = tid; t < 2 * p.L + 1; t += 128) etal[t] = p.eta[t];
}
// The thread's column and its rows k0 .. k1 - 1 of 0 .. rows - 1 (the two wavefronts of a workgroup: two segments of the same
// columns); false: nothing to do
__device__ __forceinline__ bool walk_segment(const KParams & p, int xmode, int ntile, int nseg, int rows, int & col, int & k0, int & k1) {
	int bx, by;
	if (!xcd_column_tile(xmode, ntile, (nseg + 1) / 2, bx, by)) return false;
	col = (p.quads ? p.quads[bx] : bx) * 64 + threadIdx.x;
	if (col >= p.ncol) return false;
	const int sg = WAVE_UNIFORM(by * 2 + (int)threadIdx.y);
	const int seg = (rows + nseg - 1) / nseg;
	k0 = sg * seg; k1 = min(rows, k0 + seg);
	return sg < nseg && k0 < k1;
}



// Ordering point for LDS rows that only ONE wavefront touches (the contraction rows s[ty][..] of the horizontal kernels, each
// wavefront's copy of the 4 x 4 operator tables): the LDS executes a wavefront's operations in order, so lanes see one another's
// writes without a workgroup barrier; the fences keep the compiler from moving reads above the writes they depend on.
__device__ __forceinline__ void wave_sync() {
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Lane of a wavefront = position e * 16 + i * 4 + j inside its tile of four elements, in every kernel, and a contraction row of LDS
// holds a tile's 64 values in that order.  In the node-unique kernels a 16-lane group is then one element = four runs of 32 bytes in
// four different rows of the slab, four times the L1 / L2 requests per load instruction of the element-major kernel (measured: 2.1 x
// its L2 requests and +12 % time for 23 % fewer bytes).  The map lane = j + 4 e + 16 i (16 consecutive lanes = one node row of the
// tile's four elements, one or two 128-byte lines) halves those requests and was measured slower: with the LDS rows as they are the
// permuted lanes cost the contractions two-way bank conflicts (hyperviscosity pass 149 -> 196 us); with rows padded to 80 doubles
// the explicit stage is level (0.577 against 0.576 ms per step) and the hyperviscosity pass 4 % slower.  Halving the L2 requests buys
// nothing (tools/experiments/kernel_build_switches.patch).
// unique-slab index of the node at position `lane` of tile `tile` (-1: padding), from the tile's eight wave-uniform table entries:
// no per-lane table load in front of the state loads (a dependent memory round trip at the head of every wavefront: the
// explicit kernels ran 12 % and the hyperviscosity pass 20 % longer with t_ucol[col] there)
__device__ __forceinline__ int tile_ucol(const KParams & p, int tile, int lane) {
	const int * ti = p.t_tinfo + (size_t)WAVE_UNIFORM(tile) * 8;
	const int e = lane >> 4;
	const int b0 = ti[0], b1 = ti[1], b2 = ti[2], b3 = ti[3], n0 = ti[4], n1 = ti[5], n2 = ti[6], n3 = ti[7];
	const int base = (e == 0) ? b0 : ((e == 1) ? b1 : ((e == 2) ? b2 : b3));
	const int nj = (e == 0) ? n0 : ((e == 1) ? n1 : ((e == 2) ? n2 : n3));
	return (base < 0) ? -1 : base + ((lane >> 2) & 3) * nj + (lane & 3);
}

// workgroup -> (entry of the launch's tile list, level block).  Element-major kernels: the plain 2-D launch.  Node-unique kernels
// (UQ): a 1-D launch unfolded so that every XCD sweeps a contiguous range of tiles, level block by level block -- neighbouring
// tiles read the same rows of the unique slabs (the nodes on their common edge), which then come from that XCD's L2.
template <bool UQ> __device__ __forceinline__ bool wg_tile(const KParams & p, int nyb, int & tile_ix, int & yb) {
	if (!UQ) { tile_ix = blockIdx.x; yb = blockIdx.y; return true; }
	if (p.u_xcd) return xcd_tile(p.u_ntiles, nyb, tile_ix, yb);
	tile_ix = blockIdx.x % p.u_ntiles; yb = blockIdx.x / p.u_ntiles;
	return yb < nyb;
}
static inline dim3 wg_grid(bool uq, const KParams & p, int ntiles, int nyb) {
	if (!uq) return dim3(ntiles, nyb);
	return dim3(p.u_xcd ? 8 * ((ntiles + 7) / 8) * nyb : ntiles * nyb);
}

// ---------------------------------------------------------------------------------------------
// Node-unique state layout (UniqueLayout, tmx_internal.h): what a thread = (element, node) does with its NV results.
//   sdst >= 0   the node belongs to this lane: store there -- after averaging with the copies other lanes of the wavefront hold,
//               in the reference's order (GridCSGLL::ApplyDSS, GridCSGLL.cpp:560-781: 0.5 (x + x'), four copies
//               0.5 (0.5 (x + x_alpha) + 0.5 (x_beta + x_diag)); inside a patch every copy would receive these very bits)
//   sdst == -1  nothing: another lane of the wavefront stores this node (or a padding lane)
//   sdst <= -2  the node's copies are not all in this wavefront (tile edge, patch edge): the per-element value goes to partial
//               slot -2 - sdst, k_dss_u finishes the node
// srow: NV rows of 64 doubles of LDS private to the wavefront.  LDS operations of one wavefront execute in order, so the
// exchange needs no workgroup barrier; the wavefront-scope fence keeps the compiler from moving the reads above the writes.
template <int NV>
__device__ __forceinline__ void seam_store(const KParams & p, double (*srow)[64], int lane, int sdst, int sred, const double (&v)[NV],
	double * __restrict__ xo, const int (&slab)[NV], int nv)
{
#pragma unroll
	for (int t = 0; t < NV; t++) if (t < nv) srow[t][lane] = v[t];
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	if (sdst == -1) return;
	const int n = sred & 15;
	double o[NV];
#pragma unroll
	for (int t = 0; t < NV; t++) o[t] = v[t];
	if (n == 2) {
		const int l1 = (sred >> 4) & 63;
#pragma unroll
		for (int t = 0; t < NV; t++) if (t < nv) o[t] = 0.5 * (v[t] + srow[t][l1]);
	} else if (n == 4) {
		const int l1 = (sred >> 4) & 63, l2 = (sred >> 10) & 63, l3 = (sred >> 16) & 63;
#pragma unroll
		for (int t = 0; t < NV; t++) if (t < nv) {
			const double p0 = v[t] + srow[t][l1], p1 = srow[t][l2] + srow[t][l3];
			o[t] = 0.5 * (0.5 * p0 + 0.5 * p1);
		}
	}
	if (sdst >= 0) {
#pragma unroll
		for (int t = 0; t < NV; t++) if (t < nv) xo[(size_t)slab[t] * p.NSS + sdst] = o[t];
	} else {
		const int q = -2 - sdst;
#pragma unroll
		for (int t = 0; t < NV; t++) if (t < nv) p.part[(size_t)slab[t] * p.NP + q] = o[t];
	}
}

// Seam exchange of a BLOCK: the workgroup's (up to) four wavefronts hold a block of the thread order; a node whose copies all sit in the
// block is averaged here (reference order, as seam_store), whichever wavefronts hold them.  xrow: [6][256] doubles of LDS shared by the
// workgroup, one of two buffers alternating by level, so that ONE barrier per level orders everything: a wavefront that writes buffer b
// for level k + 2 has passed the barrier of level k + 1, which every wavefront reaches only after its reads of level k (buffer b).
// The barrier waits for LDS traffic only (s_waitcnt lgkmcnt(0)): __syncthreads() would also drain vmcnt, i.e. wait for the prefetched
// next level and the combination's terms in flight -- the very loads the walk issues early.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int NV>
__device__ __forceinline__ void block_seam_store(const KParams & p, double (*xrow)[256], int pos, int sdst, int sred, const double (&v)[NV],
	double * __restrict__ xo, const int (&slab)[NV], unsigned vmask)
{
#pragma unroll
	for (int t = 0; t < NV; t++) if ((vmask >> t) & 1u) xrow[t][pos] = v[t];
	lds_barrier();
	if (sdst == -1) return;
	const int n = sred & 15;
	double o[NV];
#pragma unroll
	for (int t = 0; t < NV; t++) o[t] = v[t];
	if (n == 2) {
		const int l1 = (sred >> 4) & 255;
#pragma unroll
		for (int t = 0; t < NV; t++) if ((vmask >> t) & 1u) o[t] = 0.5 * (v[t] + xrow[t][l1]);
	} else if (n == 4) {
		const int l1 = (sred >> 4) & 255, l2 = (sred >> 12) & 255, l3 = (sred >> 20) & 255;
#pragma unroll
		for (int t = 0; t < NV; t++) if ((vmask >> t) & 1u) {
			const double p0 = v[t] + xrow[t][l1], p1 = xrow[t][l2] + xrow[t][l3];
			o[t] = 0.5 * (0.5 * p0 + 0.5 * p1);
		}
	}
	if (sdst >= 0) {
#pragma unroll
		for (int t = 0; t < NV; t++) if ((vmask >> t) & 1u) xo[(size_t)slab[t] * p.NSS + sdst] = o[t];
	} else {
		const int q = -2 - sdst;
#pragma unroll
		for (int t = 0; t < NV; t++) if ((vmask >> t) & 1u) p.part[(size_t)slab[t] * p.NP + q] = o[t];
	}
}
