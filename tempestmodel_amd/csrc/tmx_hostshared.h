// tmx_hostshared.h -- what the host-side translation units share: tmx_host.hip (C ABI set-up: life cycle, patches, state transfer,
// restart image, communicator set-up, introspection), tmx_plan.hip (tmx_finalize: the plan of a rank built on the host, then uploaded;
// plan introspection), tmx_options.hip (the option table and its four entry points), tmx_step.hip (the operations on the resident
// state: stage algebra, the explicit stage and the hyperviscosity passes with their boundary-first loop, exchange, interpolation, column
// physics), tmx_program.hip (the stepper programs:
// builder, matcher of fused units, access analysis, the element-major and node-unique interpreters, tmx_step) and tmx_unique.hip
// (the node-unique layout: its tables and their upload).  Also here: gather_terms, the one place where a coefficient vector becomes the ordered terms of a stage (StageTerms).
#pragma once
#include "tmx_internal.h"
#include <pthread.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <map>
#include <mutex>
#include <numeric>
#include <functional>
#include <thread>

static inline bool plan_only(const tmx_engine * e) { return e->cfg.device == -2; }

// RCCL, resolved at run time so the library loads without it (single-GPU use, CPU symbol checks)
typedef struct { char internal[128]; } nccl_uid;
typedef int (*fn_ncclGetUniqueId)(nccl_uid *);
typedef int (*fn_ncclCommInitRank)(void **, int, nccl_uid, int);
typedef int (*fn_ncclCommDestroy)(void *);
typedef int (*fn_ncclGroupStart)(void);
typedef int (*fn_ncclGroupEnd)(void);
typedef int (*fn_ncclSend)(const void *, size_t, int, int, void *, hipStream_t);
typedef int (*fn_ncclRecv)(void *, size_t, int, int, void *, hipStream_t);
typedef const char * (*fn_ncclGetErrorString)(int);
typedef int (*fn_ncclCommCount)(void *, int *);

struct NcclApi {
	void * lib = nullptr;
	fn_ncclGetUniqueId GetUniqueId = nullptr;
	fn_ncclCommInitRank CommInitRank = nullptr;
	fn_ncclCommDestroy CommDestroy = nullptr;
	fn_ncclGroupStart GroupStart = nullptr;
	fn_ncclGroupEnd GroupEnd = nullptr;
	fn_ncclSend Send = nullptr;
	fn_ncclRecv Recv = nullptr;
	fn_ncclGetErrorString GetErrorString = nullptr;
	fn_ncclCommCount CommCount = nullptr;
};
extern NcclApi g_nccl;

int load_rccl();
#define NCCLCHK(call) do { int _r = (call); if (_r != 0) { \
	tmx_set_error("%s failed: %s", #call, g_nccl.GetErrorString ? g_nccl.GetErrorString(_r) : "?"); return TMX_ERR_COMM; } } while (0)

// ---------------------------------------------------------------------------------------------
// profiling helper: bracket a launch sequence with events on the engine's stream

struct ProfScope {
	tmx_engine * e; int id; hipEvent_t a = nullptr, b = nullptr;
	ProfScope(tmx_engine * e_, int id_) : e(e_), id(id_) {
		if (e->prof) { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, e->stream); }
	}
	~ProfScope() {
		if (e->prof) { hipEventRecord(b, e->stream); e->prof_pending.push_back({ id, { a, b } }); }
	}
};

void prof_collect(tmx_engine * e);

// host vector -> a device buffer of its own (one element at least), added to the engine's byte count
template <class T> static int dev_upload(T ** d, const std::vector<T> & h, size_t * bytes) {
	const size_t n = h.size() ? h.size() : 1;
	HIPCHK(hipMalloc((void **)d, n * sizeof(T)));
	if (h.size()) HIPCHK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
	*bytes += n * sizeof(T);
	return TMX_OK;
}

// column index of local node (i,j) (reference patch-local indices, 1-based interior) of a local patch
static inline int col_of(const PatchInfo & P, int i, int j) {
	const int a = (i - 1) / TMX_NP, ii = (i - 1) % TMX_NP, b = (j - 1) / TMX_NP, jj = (j - 1) % TMX_NP;
	return (P.elem_base + a * P.neb + b) * TMX_NQ + ii * TMX_NP + jj;
}


static inline size_t p2p_header_bytes(int n_ranks) { return (((size_t)2 * n_ranks * sizeof(unsigned long long)) + 255) / 256 * 256; }

// defined in tmx_step.hip
KParams make_params(const tmx_engine * e);
int launch_check(const char * what);
int settle_instance(tmx_engine * e, int ix, bool read_only = false);
int check_ready(tmx_engine * e);
int check_inst(tmx_engine * e, int ix, bool read_only = false);
double * inst(tmx_engine * e, int ix);
void interp_orphan(tmx_engine * e);      // output-interpolation plans of an engine that is being destroyed
// ... the operations the stepper programs (tmx_program.hip) launch, and the slot bookkeeping they share with the physics entry points
const double * inst_uv(tmx_engine * e, int ix);
void drop_readers(tmx_engine * e, int x);
double * uinst(tmx_engine * e, int ix);
const double * uinst_uv(tmx_engine * e, int ix);
int u_own_uv(tmx_engine * e, int ix, bool total = false);
void u_written(tmx_engine * e, int x);
int surface_copy(tmx_engine * e, int src, int dst);
int surface_zero(tmx_engine * e, int ix);
int surface_lincomb(tmx_engine * e, const double * coeff, int n_coeff, int dst);
bool stage_can_split(const tmx_engine * e);
bool hypervis_active(const tmx_engine * e);
int hv_stage(tmx_engine * e, int iinit, int ibase, int iupd, double dt, const double * lc, int nlc, bool split);
int sw_stage(tmx_engine * e, int iinit, int ibase, int iupd, double dt, bool split);
void hvis_laplacians(tmx_engine * e, const KParams & p, const double * a, double * w);
void hvis_apply(tmx_engine * e, const KParams & p, const double * w, const double * a, double * b, double dt, bool pull_dss = false);
int copy_uv(tmx_engine * e, int src, int dst);
int v_step_implicit_impl(tmx_engine * e, int iinit, int iupd, double dt, int itbase);
int h_step_after_subcycle_impl(tmx_engine * e, int iinit, int iupd, int iwork, double dt, bool work_is_scratch);
int exchange(tmx_engine * e, const KParams & p, double * x, bool * overlapped = nullptr);
int dss_after_exchange(tmx_engine * e, const KParams & p, int ix, bool overlapped, int g_first = 0);
// defined in tmx_host.hip
int check_reference_state(tmx_engine * e);
int ensure_layout(tmx_engine * e);
int column_physics_levels(tmx_engine * e);
struct LoopbackGroup;

// Where instance m and its U,V slabs live; the return value is the instance's bit of StageTerms::dmask.  Element-major slots ...
struct WhereD {
	tmx_engine * e;
	bool operator()(int m, const double *& x, const double *& x_uv) const { x = inst(e, m); x_uv = inst_uv(e, m); return false; }
};
// ... and node-unique ones, or the element-major slot read copy by copy for an instance of `dlive`
struct WhereU {
	tmx_engine * e; unsigned dlive;
	bool operator()(int m, const double *& x, const double *& x_uv) const {
		if (dlive >> m & 1u) { WhereD{ e }(m, x, x_uv); return true; }
		x = uinst(e, m); x_uv = uinst_uv(e, m); return false;
	}
};
// the plain base instance m (StageTerms::n == 0)
template <class W> static StageTerms base_terms(int m, W where) {
	StageTerms t;
	if (where(m, t.src[0], t.src_uv[0])) t.dmask = 1u;
	return t;
}
// The combination coeff[0, n_coeff) -> dst in the reference's accumulation order (GridPatch::LinearCombineData): the destination's own term,
// then the non-zero coefficients by ascending instance index, the instances of `held` left out.  false: more than 11 source terms.
template <class W> static bool gather_terms(StageTerms & t, const double * coeff, int n_coeff, int dst, unsigned held, W where) {
	t = base_terms(dst, where);
	t.n = 1; t.coef[0] = coeff[dst]; t.premul = (coeff[dst] != 0.0) ? 1 : 0;
	for (int m = 0; m < n_coeff; m++) {
		if (m == dst || coeff[m] == 0.0 || (held >> m & 1u)) continue;
		if (t.n >= 12) return false;
		if (where(m, t.src[t.n], t.src_uv[t.n])) t.dmask |= 1u << t.n;
		t.coef[t.n++] = coeff[m];
	}
	return true;
}
