// tmx_step.hip -- host side of the engine, part 2: the operations on the resident state -- stage algebra, the dynamics entry points, the
// explicit stage (hv_stage, sw_stage) and the two hyperviscosity passes (hvis_laplacians, hvis_apply), the boundary-first loop they run in on
// several ranks (produce_and_average), DSS + exchange, output interpolation, column physics.  (Part 1, set-up and transfers: tmx_host.hip;
// part 3, the stepper programs and their interpreters: tmx_program.hip; shared declarations and the gatherer of a stage's terms: tmx_hostshared.h.)
#include "tmx_hostshared.h"

// ---------------------------------------------------------------------------------------------
// kernel parameter block

KParams make_params(const tmx_engine * e) {
	KParams p;
	p.L = e->L; p.ncol = e->ncol; p.NS = e->NS;
	p.g2d = e->d_g2d; p.g3n = e->d_g3n; p.g3e = e->d_g3e; p.ops = e->d_ops;
	p.eta = e->d_eta; p.closed = e->metric_closed ? 1 : 0;
	p.inv_da = 1.0 / e->cfg.element_delta_a;
	p.quads = nullptr;      // all tiles (a boundary-first launch names its tile list: produce_and_average)
	p.NSS = e->NS; p.t_ucol = nullptr; p.t_tinfo = nullptr; p.t_sdst = nullptr; p.t_sred = nullptr; p.part = nullptr; p.NP = 0;      // element-major layout (tmxu_params: node-unique)
	p.u_ntiles = 0; p.u_xcd = e->u.xcd_order;
	p.NSD = e->NS; p.t_dcol = nullptr; p.b_sdst = nullptr; p.b_sred = nullptr; p.blk_info = nullptr; p.bquads = nullptr;
	p.grav = e->cfg.grav; p.Rd = e->cfg.Rd; p.cp = e->cfg.cp; p.p0 = e->cfg.p0;
	memcpy(p.dx, e->h_dx, sizeof(p.dx)); memcpy(p.stiff, e->h_stiff, sizeof(p.stiff));
	return p;
}

int check_ready(tmx_engine * e) {
	REQUIRE(e && e->finalized && !plan_only(e), TMX_ERR_INVALID, "engine not finalized");
	return TMX_OK;
}
int check_inst(tmx_engine * e, int ix, bool read_only) {
	REQUIRE(ix >= 0 && ix < e->cfg.n_instances, TMX_ERR_INVALID, "instance %d out of range [0,%d)", ix, e->cfg.n_instances);
	return settle_instance(e, ix, read_only);
}
double * inst(tmx_engine * e, int ix) { return e->d_state + (size_t)e->imap[ix] * e->inst_stride; }
// where the U,V slabs of an instance live (the first 2 L slabs of a slot): its slot, or the slot it shares U,V with
const double * inst_uv(tmx_engine * e, int ix) { return e->d_state + (size_t)(e->uvmap[ix] != ix ? e->uvmap[ix] : e->imap[ix]) * e->inst_stride; }
// Entry points other than tmx_step see the instances they name in slots of their own: an instance that reads another one's
// slot, or whose slot others read (b == ix or imap[b] == ix), gets the CopyData that was left out.  b < 0: all of them.
// Shared U,V slabs are settled inside a stepper program too: the operations that understand them (the fused explicit stage)
// do not come through here.
// read_only: the caller only reads instance ix (downloads, output interpolation, the restart image).  The node-unique form of an
// instance converted for a reader stays valid beside the element-major one (form 2), so a download between two steps costs one
// conversion of the instance read and the next tmx_step neither checks nor converts anything.
int settle_instance(tmx_engine * e, int ix, bool read_only) {
	// slots in node-unique form (left by tmx_step) go back to the element-major form before anything else looks at them: the one
	// named (where nothing shares slots), else all of them; a writer invalidates the node-unique copy
	if (e->u.n_uform) {
		bool one = ix >= 0 && e->imap[ix] == ix && e->uvmap[ix] == ix;
		for (int b = 0; b < (int)e->imap.size() && one; b++) if (b != ix && (e->imap[b] == ix || e->uvmap[b] == ix)) one = false;
		for (int b = 0; b < (int)e->u.form.size(); b++)
			if (e->u.form[b] && (!one || b == ix)) { int r = tmxu_to_d(e, b, one && read_only); if (r) return r; }
	}
	if (e->n_shared && !e->in_program)
		for (int b = 0; b < (int)e->imap.size(); b++) {
			if (e->imap[b] == b || !(ix < 0 || b == ix || e->imap[b] == ix)) continue;
			HIPCHK(hipMemcpyAsync(e->d_state + (size_t)b * e->inst_stride, e->d_state + (size_t)e->imap[b] * e->inst_stride,
				e->inst_stride * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
			e->imap[b] = b; e->n_shared--;
		}
	if (e->n_uvshared)
		for (int b = 0; b < (int)e->uvmap.size(); b++) {
			if (e->uvmap[b] == b || !(ix < 0 || b == ix || e->uvmap[b] == ix)) continue;
			HIPCHK(hipMemcpyAsync(e->d_state + (size_t)b * e->inst_stride, e->d_state + (size_t)e->uvmap[b] * e->inst_stride,
				(size_t)2 * e->L * e->NS * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
			e->uvmap[b] = b; e->n_uvshared--;
		}
	return TMX_OK;
}

// instance x has been written: the instances that read its slot (or its U,V slabs) are dead by share_is_safe (tmx_program.hip) and go
// back to their own
void drop_readers(tmx_engine * e, int x) {
	for (int y = 0; y < (int)e->imap.size(); y++) {
		if (y != x && e->imap[y] == x) { e->imap[y] = y; e->n_shared--; }
		if (y != x && e->uvmap[y] == x) { e->uvmap[y] = y; e->n_uvshared--; }
	}
}
// the same slots on the node-unique layout (UniqueLayout, tmx_internal.h)
double * uinst(tmx_engine * e, int ix) { return e->u.d_ustate + (size_t)e->u.uslot[ix] * e->u.ustride; }
// U,V slabs of an instance: its own slot, or the slot of the instance it shares them with (tmx_engine::uvmap, the rules of the
// element-major programs: the Copy in front of the column solve leaves the copy's U,V identical to the source's)
const double * uinst_uv(tmx_engine * e, int ix) { return uinst(e, e->uvmap[ix]); }
// instance ix is about to be read through ONE pointer (or updated in place): give it its own U,V slabs
int u_own_uv(tmx_engine * e, int ix, bool total) {
	if (e->uvmap[ix] == ix) return TMX_OK;
	if (!total) {
		ProfScope ps(e, TMX_K_LINCOMB);
		HIPCHK(hipMemcpyAsync(uinst(e, ix), uinst_uv(e, ix), (size_t)2 * e->L * e->u.NUS * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
	}
	e->uvmap[ix] = ix; e->n_uvshared--;
	return TMX_OK;
}
// instance x has been rewritten: whoever read its U,V slabs is dead by share_is_safe
void u_written(tmx_engine * e, int x) { if (e->n_uvshared) drop_readers(e, x); }

// Surface slots.  HeldSuarezPhysics::Perform forms its "surface pressure" from dataREdge[RIx][i][j][0] *
// dataREdge[TIx][i][j][0] (HeldSuarezPhysics.cpp:113-116).  With Lorenz staggering rho and rho*theta live on levels and
// those interface entries are scratch: the test case fills them and afterwards ONLY Grid::CopyData / ZeroData /
// LinearCombineData -- which run over whole arrays (GridPatch.cpp:1402-1553) -- change them, by a rounding error per
// combination.  To reproduce the forcing bit for bit the engine carries the two entries per column through the same
// stage algebra: they sit behind the state of every instance, whole-instance copies / combinations include them for
// free, and the fused paths below (which never materialise the copy or combination) update them separately -- only
// when a caller asked for tracked surface slots (tmx_set_patch_physics_inputs with surface_pressure == NULL).
static double * surface_slots(tmx_engine * e, int ix) { return inst(e, ix) + (size_t)e->nslab * e->NS; }
int surface_copy(tmx_engine * e, int src, int dst) {
	if (!e->track_surface || src == dst) return TMX_OK;
	HIPCHK(hipMemcpyAsync(surface_slots(e, dst), surface_slots(e, src), (size_t)2 * e->NS * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
	return TMX_OK;
}
int surface_zero(tmx_engine * e, int ix) {
	if (!e->track_surface) return TMX_OK;
	HIPCHK(hipMemsetAsync(surface_slots(e, ix), 0, (size_t)2 * e->NS * sizeof(double), e->stream));
	return TMX_OK;
}
// (the surface slots live with the element-major slots, whatever layout the stage ran on)
int surface_lincomb(tmx_engine * e, const double * coeff, int n_coeff, int dst) {
	if (!e->track_surface) return TMX_OK;
	StageTerms t;
	REQUIRE(gather_terms(t, coeff, n_coeff, dst, 0u, WhereD{ e }), TMX_ERR_UNSUPPORTED, "linear combination with more than 11 source terms");
	tmxk_lincomb(e, (size_t)2 * e->NS, surface_slots(e, dst), terms_at(t, (size_t)e->nslab * e->NS));
	return TMX_OK;
}

int launch_check(const char * what) {
	hipError_t r = hipGetLastError();
	if (r != hipSuccess) { tmx_set_error("%s: %s", what, hipGetErrorString(r)); return TMX_ERR_DEVICE; }
	return TMX_OK;
}

// ---------------------------------------------------------------------------------------------
// stage algebra

extern "C" int tmx_copy_data(tmx_engine * e, int src, int dst) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, src)) || (r = check_inst(e, dst))) return r;
	if (src == dst) return TMX_OK;
	ProfScope ps(e, TMX_K_LINCOMB);
	HIPCHK(hipMemcpyAsync(inst(e, dst), inst(e, src), e->inst_stride * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
	return TMX_OK;
}

extern "C" int tmx_zero_data(tmx_engine * e, int ix) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, ix))) return r;
	HIPCHK(hipMemsetAsync(inst(e, ix), 0, e->inst_stride * sizeof(double), e->stream));
	return TMX_OK;
}

extern "C" int tmx_linear_combine_data(tmx_engine * e, const double * coeff, int n_coeff, int dst) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, dst))) return r;
	REQUIRE(coeff && n_coeff > dst && n_coeff <= e->cfg.n_instances, TMX_ERR_INVALID,
		"linear_combine_data: %d coefficients for destination %d and %d instances", n_coeff, dst, e->cfg.n_instances);
	if ((r = settle_instance(e, -1, false))) return r;
	StageTerms t;
	REQUIRE(gather_terms(t, coeff, n_coeff, dst, 0u, WhereD{ e }), TMX_ERR_UNSUPPORTED, "linear_combine_data: more than 11 source terms");
	ProfScope ps(e, TMX_K_LINCOMB);
	tmxk_lincomb(e, e->inst_stride, inst(e, dst), t);
	return launch_check("lincomb");
}

// ---------------------------------------------------------------------------------------------
// dynamics

// uniform-diffusion extras at the end of HorizontalDynamicsFEM::StepExplicit (:1817-1859)
// fused: the explicit stage's kernel has applied it already (tmxk_h_walk_fuses_udiff)
static int h_uniform_diffusion(tmx_engine * e, const KParams & p, int iinit, int iupd, double dt, bool fused = false) {
	if (!e->udiff || fused) return TMX_OK;
	int r; if ((r = check_reference_state(e))) return r;
	tmxk_uniform_diffusion(e, p, inst(e, iinit), e->d_ref, inst(e, iupd), dt, e->cfg.uniform_diffusion_scalar, e->cfg.uniform_diffusion_vector);
	return TMX_OK;
}

// VerticalDynamicsFEM::StepExplicit beyond the upwind penalty of U,V (which tmxk_v_explicit / the fused explicit kernel
// apply): in the fully explicit mode -dt F on rho*theta, W, rho (:745-790) and the explicit tracer update (:792-800),
// and with uniform diffusion the vertical diffusion of U,V (:1059-1105).
// uv_done: the vertical diffusion of U,V has been added by tmxk_v_explicit already (TMX_UDV_SEPARATE=1 keeps the separate pass)
static bool udv_fused(const tmx_engine * e) { return e->udiff && e->fully_explicit && !e->opt_udv_separate; }
// TMX_VX_FUSED=1: the U,V update of V.StepExplicit evaluated by the kernel of the explicitly treated implicit terms (one launch
// less, shared operands).  Off by default: config 4's step measured 4.81 ms with it, 4.75 ms without -- the terms kernel is
// bound by its dependent arithmetic, the U,V update on its own by bandwidth, and the two overlap better as two launches.
static bool uvx_fused(const tmx_engine * e) { return udv_fused(e) && e->opt_vx_fused; }
static int v_explicit_extras(tmx_engine * e, const KParams & p, int iinit, int iupd, double dt, bool uv_done = false, bool with_uv = false) {
	if (!e->fully_explicit) return TMX_OK;
	int r; if ((r = check_reference_state(e))) return r;
	tmxk_vi_terms_explicit(e, p, inst(e, iinit), inst(e, iupd), dt, with_uv);
	if (e->nt > 0)      // (the caller has asked tmx_vertical_fit before its first kernel)
		REQUIRE(tmxk_vi_tracers_explicit(e, p, inst(e, iinit), inst(e, iupd), dt) == 0, TMX_ERR_UNSUPPORTED,
			"tracer column update: %d levels do not fit the LDS working set", e->L);
	if (e->udiff && !uv_done)
		tmxk_v_uniform_diffusion_uv(e, p, inst(e, iinit), e->d_ref, inst(e, iupd), dt, e->cfg.uniform_diffusion_vector / (e->cfg.ztop * e->cfg.ztop));
	return TMX_OK;
}

extern "C" int tmx_h_step_explicit(tmx_engine * e, int iinit, int iupd, double dt) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, iinit)) || (r = check_inst(e, iupd))) return r;
	// same precondition as the reference (HorizontalDynamicsFEM.cpp:1793-1796)
	REQUIRE(iinit != iupd, TMX_ERR_INVALID, "StepExplicit: initial and update data instance must be distinct");
	ProfScope ps(e, TMX_K_H_EXPLICIT);
	const KParams p = make_params(e);
	const bool udf = !e->sw && tmxk_h_walk_fuses_udiff(e, p, 0, 0);
	if (udf && (r = check_reference_state(e))) return r;
	const StageTerms base = base_terms(iupd, WhereD{ e });      // in place
	if (e->sw) tmxk_sw_explicit(e, p, inst(e, iinit), inst(e, iupd), inst(e, iupd), dt);
	else tmxk_h_explicit(e, p, { inst(e, iinit), inst(e, iinit), inst(e, iupd), dt, 0, base, nullptr });
	if (e->nt > 0) tmxk_h_tracers(e, p, inst(e, iinit), inst(e, iinit), base, inst(e, iupd), dt);
	if ((r = h_uniform_diffusion(e, p, iinit, iupd, dt, udf))) return r;
	return launch_check("h_step_explicit");
}

// LinearCombineData(coeff -> d) + H.StepExplicit(i, d) + V.StepExplicit(i, d) in one pass: the combination is
// evaluated inside the kernels (same accumulation order), the combined state is never written and re-read.
// the kernels of one explicit stage (H + tracers + uniform diffusion + V) over the tiles p selects: all of them, or the tile
// list of a boundary-first stage.  base.n > 0: the update starts from that combination, else from the instance base.src[0].
static int hv_stage_kernels(tmx_engine * e, const KParams & p, int iinit, int iupd, double dt, const StageTerms & base) {
	int r;
	const int n = base.n;
	// U,V slabs that live in another instance's slot are understood by k_h_explicit and k_h_tracers only; the kernels of the other configurations
	// read them through the instance pointer, and the stepper never shares U,V there
	REQUIRE(!e->n_uvshared || (!e->udiff && !e->fully_explicit && !e->sw), TMX_ERR_UNSUPPORTED, "internal: shared U,V slabs in a configuration whose kernels do not take them");
	// with uniform diffusion the horizontal diffusion of U,V precedes the vertical penalty, as in the reference: V.StepExplicit's U,V part is
	// fused in only where the same kernel applies that diffusion first (the walk, option h_walk_udiff = 2)
	const bool uvx = uvx_fused(e);
	const bool vfu = e->udiff && !uvx && tmxk_h_walk_fuses_udiff(e, p, 1, n);
	const int fv = e->udiff ? (vfu ? 1 : 0) : 1;
	const bool udf = vfu || tmxk_h_walk_fuses_udiff(e, p, fv, n);
	if (udf && (r = check_reference_state(e))) return r;
	tmxk_h_explicit(e, p, { inst(e, iinit), inst_uv(e, iinit), inst(e, iupd), dt, fv, base, nullptr });
	if (e->nt > 0) {
		// tracers: the combination of the tracer slabs is evaluated inside the tracer kernel, which updates in place
		// (TMX_TRACER_LINCOMB_PASS=1: formed by a separate pass first, for A/B and tests; whole patches only)
		if (n > 0 && e->opt_tracer_lincomb_pass) {
			const size_t off = (size_t)(5 * e->L + 1) * e->NS, cnt = (size_t)e->nt * e->L * e->NS;
			tmxk_lincomb(e, cnt, inst(e, iupd) + off, terms_at(base, off));
			tmxk_h_tracers(e, p, inst(e, iinit), inst_uv(e, iinit), base_terms(iupd, WhereD{ e }), inst(e, iupd), dt);
		} else
			tmxk_h_tracers(e, p, inst(e, iinit), inst_uv(e, iinit), base, inst(e, iupd), dt);
	}
	if ((r = h_uniform_diffusion(e, p, iinit, iupd, dt, udf))) return r;
	if (e->udiff && !uvx && !vfu) {
		if (udv_fused(e) && (r = check_reference_state(e))) return r;
		tmxk_v_explicit(e, p, inst(e, iinit), inst(e, iupd), dt, udv_fused(e));
	}
	return v_explicit_extras(e, p, iinit, iupd, dt, udv_fused(e), uvx);
}

// Fill instance ix and average it, on several ranks, boundary first: the kernels on the tiles that hold columns other
// ranks need, pack + grouped send/recv on the exchange stream, the same kernels on the remaining tiles while the wire is busy,
// then the averaging (local groups, wait for the wire, groups with remote members).  Same kernels on disjoint tiles -- every
// kernel that comes through here is local to a 64-column tile (whole elements, whole columns) -- so the result is bit-identical
// to one launch over all tiles (the form of u_produce_and_average, tmx_program.hip).  kernels(KParams) -> int: the launches, over the tile list of the KParams; tail() -> int: what
// else the operation does before `what` is checked and the averaging starts.  average = false: no DSS, only the wait for the wire.
template <class F, class G> static int produce_and_average(tmx_engine * e, int ix, int prof_slot, const char * what, F kernels, G tail, bool average = true) {
	KParams p = make_params(e);
	bool overlapped = false;
	int r;
	for (int part = 0; part < 2; part++) {
		p.quads = part ? e->d_quads_late : e->d_quads_early;
		e->launch_tiles = part ? e->n_quads_late : e->n_quads_early;
		{ ProfScope ps(e, prof_slot); r = kernels(p); }
		p.quads = nullptr;
		if (r || (part == 0 && (r = exchange(e, p, inst(e, ix), &overlapped)))) return r;
	}
	if ((r = tail()) || (r = launch_check(what))) return r;
	if (average) return dss_after_exchange(e, p, ix, overlapped);
	if (overlapped) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_recv, 0));      // the neighbours' values are in the ghost buffer
	return TMX_OK;
}
static int no_tail() { return TMX_OK; }

// The two whole-patch debug variants of the tracer kernels (TMX_VT_COLUMN, TMX_TRACER_LINCOMB_PASS) switch the boundary-first loop off.
bool stage_can_split(const tmx_engine * e) {
	return e->split_stage && !e->opt_vt_column && !e->opt_tracer_lincomb_pass;
}

// One explicit stage, [CopyData(ibase -> iupd) | LinearCombineData(lc -> iupd)] + H.StepExplicit + V.StepExplicit(iinit, iupd), in one
// pass over the state: `ibase` is the instance the update starts from (== iupd for the reference's in-place accumulation, else
// the source of the folded CopyData); lc != null: it starts from that combination instead.  Bit-identical to the separate calls.
// split: the DSS of iupd that follows is part of the call, boundary tiles first.  All configurations: plain dynamics, tracers,
// uniform diffusion, the fully explicit vertical mode (BASELINE config 4).
int hv_stage(tmx_engine * e, int iinit, int ibase, int iupd, double dt, const double * lc, int nlc, bool split) {
	StageTerms base;
	int rf; if (e->fully_explicit && (rf = tmx_vertical_fit(e, TMX_FIT_VT_EXPLICIT))) return rf;      // refusal before the stage's first kernel
	if (lc) REQUIRE(gather_terms(base, lc, nlc, iupd, 0u, WhereD{ e }), TMX_ERR_UNSUPPORTED, "linear combination with more than 11 source terms");
	else base = base_terms(ibase, WhereD{ e });
	auto kernels = [&](const KParams & p) { return hv_stage_kernels(e, p, iinit, iupd, dt, base); };
	// the surface slots of the folded combination or CopyData(base -> update)
	auto surface = [&]() { return lc ? surface_lincomb(e, lc, nlc, iupd) : surface_copy(e, ibase, iupd); };
	if (split) return produce_and_average(e, iupd, TMX_K_H_EXPLICIT, "hv_stage_split", kernels, surface);
	ProfScope ps(e, TMX_K_H_EXPLICIT);
	int r;
	if ((r = kernels(make_params(e))) || (r = surface())) return r;
	return launch_check(lc ? "hv_step_explicit(lincomb)" : "hv_step_explicit");
}

// the same for the shallow-water set, whose stage is H.StepExplicit (V is a stub); no tracked surface slots there
int sw_stage(tmx_engine * e, int iinit, int ibase, int iupd, double dt, bool split) {
	auto kernels = [&](const KParams & p) { tmxk_sw_explicit(e, p, inst(e, iinit), inst(e, ibase), inst(e, iupd), dt); return TMX_OK; };
	if (split) return produce_and_average(e, iupd, TMX_K_H_EXPLICIT, "sw_stage_split", kernels, no_tail);
	ProfScope ps(e, TMX_K_H_EXPLICIT);
	kernels(make_params(e));
	return launch_check("sw copy + H");
}

// CopyData restricted to the U,V slabs: the implicit step overwrites rho*theta, W, rho of every column
int copy_uv(tmx_engine * e, int src, int dst) {
	ProfScope ps(e, TMX_K_LINCOMB);
	// (the source's U,V slabs may live in another instance's slot: inst_uv, not inst)
	HIPCHK(hipMemcpyAsync(inst(e, dst), inst_uv(e, src), (size_t)2 * e->L * e->NS * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
	return surface_copy(e, src, dst);
}

extern "C" int tmx_v_step_explicit(tmx_engine * e, int iinit, int iupd, double dt) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, iinit)) || (r = check_inst(e, iupd))) return r;
	if (e->sw) return TMX_OK;      // VerticalDynamicsStub
	REQUIRE(iinit != iupd, TMX_ERR_INVALID, "V StepExplicit: initial and update data instance must be distinct");
	if (e->fully_explicit && (r = tmx_vertical_fit(e, TMX_FIT_VT_EXPLICIT))) return r;      // refusal before the first kernel: the update instance stays as it is
	ProfScope ps(e, TMX_K_V_EXPLICIT);
	if (udv_fused(e) && (r = check_reference_state(e))) return r;
	tmxk_v_explicit(e, make_params(e), inst(e, iinit), inst(e, iupd), dt, udv_fused(e));
	if ((r = v_explicit_extras(e, make_params(e), iinit, iupd, dt, udv_fused(e)))) return r;
	return launch_check("v_step_explicit");
}

// itbase: instance whose tracer densities the column update is subtracted from (the update instance in the
// reference; the initial instance when the CopyData in front of the call was folded away)
int v_step_implicit_impl(tmx_engine * e, int iinit, int iupd, double dt, int itbase) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, iinit)) || (r = check_inst(e, iupd))) return r;
	if (e->sw) return TMX_OK;      // VerticalDynamicsStub
	REQUIRE(dt != 0.0, TMX_ERR_INVALID, "StepImplicit: dt must be non-zero");
	// refusal before the first kernel (the column solve rewrites the update instance; the tracer update follows it): the instance stays as it is
	if ((r = tmx_vertical_fit(e, TMX_FIT_VI | TMX_FIT_VT))) return r;
	KParams p = make_params(e);
	const double * w0 = inst(e, iinit) + (size_t)TMX_SLAB_W(e->L, 0) * e->NS;
	if (e->nt > 0 && iinit == iupd) {
		// in place: the state kernel overwrites W, the tracer update needs the initial one (m_dColumnState)
		HIPCHK(hipMemcpyAsync(e->d_w0, w0, (size_t)(e->L + 1) * e->NS * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
		w0 = e->d_w0;
	}
#if TMX_EXP
	if (e->vi_mode == 1) {
		{ ProfScope ps(e, TMX_K_VI_ASSEMBLE); tmxk_vi_assemble(e, p, inst(e, iinit), dt); }
		{ ProfScope ps(e, TMX_K_VI_SOLVE); tmxk_vi_solve(e, p, inst(e, iinit), inst(e, iupd)); }
	} else
#endif
	{
		ProfScope ps(e, TMX_K_VI_SOLVE); tmxk_vi_fused(e, p, inst(e, iinit), inst(e, iupd), dt);
	}
	if (e->nt > 0) {
		// UpdateColumnTracers with the updated W, duplicates, then VerticalDynamicsFEM::FilterNegativeTracers
		ProfScope ps(e, TMX_K_VI_SOLVE);
		REQUIRE(tmxk_vi_tracers(e, p, inst(e, iinit), w0, inst(e, itbase), inst(e, iupd), dt) == 0, TMX_ERR_UNSUPPORTED,
			"tracer column update: %d levels do not fit the LDS working set", e->L);
		tmxk_v_filter_tracers(e, p, inst(e, iupd));
	}
	return launch_check("v_step_implicit");
}

extern "C" int tmx_v_step_implicit(tmx_engine * e, int iinit, int iupd, double dt) {
	if (e && e->fully_explicit) {      // VerticalDynamicsFEM::StepImplicit, :1239-1242: nothing to do
		int r; if ((r = check_ready(e)) || (r = check_inst(e, iinit)) || (r = check_inst(e, iupd))) return r;
		return TMX_OK;
	}
	return v_step_implicit_impl(e, iinit, iupd, dt, iupd);
}

// test hook (tmx_debug_loopback_group): rank engines of one process, one host thread each
struct LoopbackGroup {
	std::vector<tmx_engine *> members;
	pthread_barrier_t barrier;
};

static int exchange_loopback(tmx_engine * e, const KParams & p, double * x) {
	LoopbackGroup * G = e->lb;
	const int n = (int)G->members.size(), me = e->cfg.rank;
	if (x) tmxk_pack(e, p, x); else tmxuk_pack(e);
	HIPCHK(hipStreamSynchronize(e->stream));
	pthread_barrier_wait(&G->barrier);                  // every member has packed
	for (int s_ = 0; s_ < n; s_++) {
		if (s_ == me) continue;
		tmx_engine * S = G->members[s_];
		const int ns = S->send_rank_off[me + 1] - S->send_rank_off[me], nr = e->recv_rank_off[s_ + 1] - e->recv_rank_off[s_];
		REQUIRE(ns == nr, TMX_ERR_INVALID, "rank %d sends %d columns to rank %d which expects %d", s_, ns, me, nr);
		if (ns == 0) continue;
		HIPCHK(hipMemcpyAsync(e->d_ghost + (size_t)e->nslab * e->recv_rank_off[s_], S->d_sendbuf + (size_t)S->nslab * S->send_rank_off[me],
			(size_t)ns * S->nslab * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
	}
	HIPCHK(hipStreamSynchronize(e->stream));
	pthread_barrier_wait(&G->barrier);                  // nobody repacks before everyone has copied
	return TMX_OK;
}

extern "C" int tmx_debug_loopback_group(tmx_engine ** engines, int n) {
	REQUIRE(engines && engines[0] && n >= 0, TMX_ERR_INVALID, "tmx_debug_loopback_group: bad argument");
	if (n == 0) {
		LoopbackGroup * G = engines[0]->lb;
		if (G) { for (tmx_engine * m : G->members) m->lb = nullptr; pthread_barrier_destroy(&G->barrier); delete G; }
		return TMX_OK;
	}
	LoopbackGroup * G = new LoopbackGroup();
	for (int a = 0; a < n; a++) {
		tmx_engine * e = engines[a];
		REQUIRE(e && e->finalized && e->cfg.n_ranks == n && e->cfg.rank == a && !e->lb, TMX_ERR_INVALID, "engine %d is not rank %d of %d (or already grouped)", a, a, n);
		G->members.push_back(e);
	}
	pthread_barrier_init(&G->barrier, nullptr, (unsigned)n);
	for (tmx_engine * m : G->members) m->lb = G;
	return TMX_OK;
}


// Exchange of the boundary columns of instance x.  ONE message per neighbour rank (the reference aggregates its
// ExchangeBuffers the same way, Connectivity.cpp:928-993): buffers are [peer][slab][count_peer], contiguous per peer.
// The grouped send/recv runs on a second stream between two events, so that the DSS of the groups without remote
// members (the great majority) overlaps the wire; *overlapped tells the caller to wait for ev_recv before the rest.
int exchange(tmx_engine * e, const KParams & p, double * x, bool * overlapped) {
	if (overlapped) *overlapped = false;
	if (e->cfg.n_ranks == 1 || (e->nsend == 0 && e->nghost == 0)) return TMX_OK;
	if (e->lb) return exchange_loopback(e, p, x);
	// timing aid: a lone rank engine of an N-rank layout with the wire left out (results are then wrong at the rank
	// boundary; used only by tools/rank_share_timing.py to measure the per-rank compute share of a step)
	if (TMX_EXP && e->opt_skip_exchange) { if (x) tmxk_pack(e, p, x); else tmxuk_pack(e); return TMX_OK; }      // (experiments flavour only)
	REQUIRE(e->comm || e->p2p, TMX_ERR_COMM, "tmx_comm_init or tmx_halo_p2p_connect must be called before a multi-rank exchange");
	ProfScope ps(e, TMX_K_EXCHANGE);
	const unsigned long long seq = ++e->p2p_seq;
	const int buf = (int)(seq & 1);
	// (x == nullptr: node-unique layout, what travels are the per-element values in the partial slots)
	if (e->p2p) { if (x) tmxk_pack_p2p(e, p, x, buf); else tmxuk_pack_p2p(e, buf); }
	else { if (x) tmxk_pack(e, p, x); else tmxuk_pack(e); }
	hipStream_t ws = e->stream;
	if (overlapped && e->xstream) {
		HIPCHK(hipEventRecord(e->ev_pack, e->stream));
		HIPCHK(hipStreamWaitEvent(e->xstream, e->ev_pack, 0));
		ws = e->xstream;
	}
	if (e->p2p) {
		// the gather has written the neighbours' ghost buffers of this parity; say so and wait for theirs.  Two parities are
		// enough: a neighbour writes parity b again only after its own averaging of the exchange in between, which needed this
		// rank's message of that exchange, which this rank sent after the averaging that read parity b.
		tmxk_p2p_signal_wait(e, ws, buf, seq);
		e->d_ghost = (double *)((char *)e->p2p_block + p2p_header_bytes(e->cfg.n_ranks)) + (size_t)buf * e->nslab * e->nghost_pad;
		if (ws != e->stream) {
			HIPCHK(hipEventRecord(e->ev_recv, ws));
			*overlapped = true;
		}
		return TMX_OK;
	}
	NCCLCHK(g_nccl.GroupStart());
	for (int rk = 0; rk < e->cfg.n_ranks; rk++) {
		const int ns = e->send_rank_off[rk + 1] - e->send_rank_off[rk], nr = e->recv_rank_off[rk + 1] - e->recv_rank_off[rk];
		if (ns) NCCLCHK(g_nccl.Send(e->d_sendbuf + (size_t)e->nslab * e->send_rank_off[rk], (size_t)ns * e->nslab, 8 /* ncclFloat64 */, rk, e->comm, ws));
		if (nr) NCCLCHK(g_nccl.Recv(e->d_ghost + (size_t)e->nslab * e->recv_rank_off[rk], (size_t)nr * e->nslab, 8, rk, e->comm, ws));
	}
	NCCLCHK(g_nccl.GroupEnd());
	if (ws != e->stream) {
		HIPCHK(hipEventRecord(e->ev_recv, ws));
		*overlapped = true;
	}
	return TMX_OK;
}

// ---- test hooks for the multi-rank device path on a single GPU ------------------------------------
// Several engines (ranks 0..n-1 of the same n-rank grid) live in ONE process on one device; the
// transport is replaced by device-to-device copies that follow exactly the wire order of the RCCL
// path (segment [send_rank_off[r], send_rank_off[r+1]) of each slab of the sender -> segment
// [recv_rank_off[s], ...) of the receiver's ghost buffer).  Packing, ghost indexing and the DSS
// kernel with remote members are the production code.
extern "C" int tmx_debug_dss_loopback(tmx_engine ** engines, int n, int ix) {
	REQUIRE(engines && n >= 1, TMX_ERR_INVALID, "tmx_debug_dss_loopback: bad argument");
	int r;
	for (int a = 0; a < n; a++) {
		tmx_engine * e = engines[a];
		if ((r = check_ready(e)) || (r = check_inst(e, ix))) return r;
		REQUIRE(e->cfg.n_ranks == n && e->cfg.rank == a, TMX_ERR_INVALID, "engine %d is rank %d of %d", a, e->cfg.rank, e->cfg.n_ranks);
		tmxk_pack(e, make_params(e), inst(e, ix));
		HIPCHK(hipStreamSynchronize(e->stream));
	}
	for (int s_ = 0; s_ < n; s_++) for (int d_ = 0; d_ < n; d_++) {
		if (s_ == d_) continue;
		tmx_engine * S = engines[s_], * D = engines[d_];
		const int ns = S->send_rank_off[d_ + 1] - S->send_rank_off[d_], nr = D->recv_rank_off[s_ + 1] - D->recv_rank_off[s_];
		REQUIRE(ns == nr, TMX_ERR_INVALID, "rank %d sends %d columns to rank %d which expects %d", s_, ns, d_, nr);
		if (ns == 0) continue;
		HIPCHK(hipMemcpy(D->d_ghost + (size_t)D->nslab * D->recv_rank_off[s_], S->d_sendbuf + (size_t)S->nslab * S->send_rank_off[d_],
			(size_t)ns * S->nslab * sizeof(double), hipMemcpyDeviceToDevice));
	}
	HIPCHK(hipDeviceSynchronize());     // device-to-device copies may still be in flight on the null stream
	for (int a = 0; a < n; a++) {
		tmx_engine * e = engines[a];
		tmxk_dss(e, make_params(e), inst(e, ix), 0, e->ngroups_local);
		tmxk_dss(e, make_params(e), inst(e, ix), e->ngroups_local, e->ngroups);
		if ((r = launch_check("dss (loopback)"))) return r;
	}
	return TMX_OK;
}

// RCCL transport self-test on one rank: a grouped send/recv to self of the send buffer into the ghost
// buffer region (library resolution, communicator, stream ordering).  Returns TMX_OK if the bytes arrive.
extern "C" int tmx_debug_comm_selftest(tmx_engine * e) {
	int r; if ((r = check_ready(e))) return r;
	REQUIRE(e->comm, TMX_ERR_COMM, "tmx_comm_init first");
	const int n = 4096;
	double * a = nullptr, * b = nullptr;
	HIPCHK(hipMalloc((void **)&a, n * sizeof(double))); HIPCHK(hipMalloc((void **)&b, n * sizeof(double)));
	std::vector<double> h(n), g(n, 0.0);
	for (int i = 0; i < n; i++) h[i] = 0.5 * i + 1.0;
	HIPCHK(hipMemcpy(a, h.data(), n * sizeof(double), hipMemcpyHostToDevice));
	HIPCHK(hipMemset(b, 0, n * sizeof(double)));
	// the choreography of exchange(): producer on the engine's stream, event, grouped send/recv on the exchange
	// stream, event, consumer back on the engine's stream -- three rounds so that buffer reuse is ordered too
	for (int round = 0; round < 3; round++) {
		HIPCHK(hipMemcpyAsync(a, h.data(), n * sizeof(double), hipMemcpyHostToDevice, e->stream));
		hipStream_t ws = e->stream;
		if (e->xstream) {
			HIPCHK(hipEventRecord(e->ev_pack, e->stream));
			HIPCHK(hipStreamWaitEvent(e->xstream, e->ev_pack, 0));
			ws = e->xstream;
		}
		NCCLCHK(g_nccl.GroupStart());
		NCCLCHK(g_nccl.Send(a, (size_t)n, 8, e->cfg.rank, e->comm, ws));
		NCCLCHK(g_nccl.Recv(b, (size_t)n, 8, e->cfg.rank, e->comm, ws));
		NCCLCHK(g_nccl.GroupEnd());
		if (e->xstream) {
			HIPCHK(hipEventRecord(e->ev_recv, ws));
			HIPCHK(hipStreamWaitEvent(e->stream, e->ev_recv, 0));
		}
		HIPCHK(hipMemcpyAsync(g.data(), b, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
		HIPCHK(hipStreamSynchronize(e->stream));
		for (int i = 0; i < n; i++) REQUIRE(g[i] == h[i], TMX_ERR_COMM, "RCCL self send/recv returned wrong data at %d (round %d)", i, round);
		for (int i = 0; i < n; i++) { h[i] = h[i] * 1.5 + round; g[i] = 0.0; }
	}
	hipFree(a); hipFree(b);
	return TMX_OK;
}

extern "C" int tmx_apply_dss(tmx_engine * e, int ix) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, ix))) return r;
	KParams p = make_params(e);
	bool overlapped = false;
	if ((r = exchange(e, p, inst(e, ix), &overlapped))) return r;
	return dss_after_exchange(e, p, ix, overlapped);
}

// the averaging after the exchange of instance ix has been started (exchange()): groups without remote members first
// g_first: first group to average (0: all; ngroups_inpatch: the producing kernel has averaged the in-patch groups itself)
int dss_after_exchange(tmx_engine * e, const KParams & p, int ix, bool overlapped, int g_first) {
	ProfScope ps(e, TMX_K_DSS);
	if (e->cfg.n_ranks > 1 && e->ngroups_local < e->ngroups) {
		// groups whose members all live on this rank first (they overlap the wire), then the ones with remote members
		tmxk_dss(e, p, inst(e, ix), g_first, e->ngroups_local);
		if (overlapped) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_recv, 0));
		tmxk_dss(e, p, inst(e, ix), e->ngroups_local, e->ngroups);
	} else {
		tmxk_dss(e, p, inst(e, ix), g_first, e->ngroups);
	}
	return launch_check("apply_dss");
}

// The two passes of the fourth-order hyperviscosity (state + tracers): w <- Laplacians of a ...
void hvis_laplacians(tmx_engine * e, const KParams & p, const double * a, double * w) {
	tmxk_hypervis(e, p, a, nullptr, w, 1.0, 1.0, 1.0, 1.0, 0);
	if (e->nt > 0) tmxk_hypervis_tracers(e, p, a, nullptr, w, 1.0, 1.0, 0, 0);
}
// ... and b <- a - dt nu Laplacians of w, the coefficients scaled with the patch's (delta_alpha / reference length)^3.2, per column (G2_NUS)
void hvis_apply(tmx_engine * e, const KParams & p, const double * w, const double * a, double * b, double dt, bool pull_dss) {
	const tmx_config & c = e->cfg;
	const int scale = (c.reference_length != 0.0) ? 1 : 0;
	tmxk_hypervis(e, p, w, a, b, -dt, c.nu_scalar, c.nu_div, c.nu_vort, scale, pull_dss);
	if (e->nt > 0) tmxk_hypervis_tracers(e, p, w, a, b, -dt, c.nu_scalar, 1, scale);
}

// work_is_scratch: the caller never looks at the working instance afterwards (the steppers' own programs); the ABI call
// leaves it as the reference does (the first pass's Laplacians, DSS'ed).
extern "C" int tmx_h_step_after_subcycle(tmx_engine * e, int iinit, int iupd, int iwork, double dt) {
	return h_step_after_subcycle_impl(e, iinit, iupd, iwork, dt, false);
}
int h_step_after_subcycle_impl(tmx_engine * e, int iinit, int iupd, int iwork, double dt, bool work_is_scratch) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, iinit)) || (r = check_inst(e, iupd)) || (r = check_inst(e, iwork))) return r;
	// preconditions of the reference (HorizontalDynamicsFEM.cpp:2648-2655)
	REQUIRE(iinit != iwork, TMX_ERR_INVALID, "StepAfterSubCycle: initial and working data must be distinct");
	REQUIRE(iupd != iwork, TMX_ERR_INVALID, "StepAfterSubCycle: working and update data must be distinct");
	const tmx_config & c = e->cfg;
	KParams p = make_params(e);
	if ((c.nu_scalar == 0.0 && c.nu_div == 0.0 && c.nu_vort == 0.0) || c.hypervis_order == 0) {
		if ((r = tmx_copy_data(e, iinit, iupd))) return r;
	} else if (c.hypervis_order == 2) {
		if ((r = surface_copy(e, iinit, iupd))) return r;       // CopyData(initial -> update), :2663-2664
		// viscosity (HorizontalDynamicsFEM.cpp:2672-2686): one pass from the initial instance, coefficients not scaled
		// with the grid spacing; the scalar part runs with +dt and the vector part with -dt, which the kernel's single
		// dt expresses exactly through the sign of nu_scalar ((-dt) * (-nu) is the same product)
		{ ProfScope ps(e, TMX_K_HYPERVIS); tmxk_hypervis(e, p, inst(e, iinit), inst(e, iinit), inst(e, iupd), -dt, -c.nu_scalar, c.nu_div, c.nu_vort, 0);
		  if (e->nt > 0) tmxk_hypervis_tracers(e, p, inst(e, iinit), inst(e, iinit), inst(e, iupd), dt, c.nu_scalar, 1, 0); }
		if ((r = launch_check("viscosity pass"))) return r;
		if ((r = tmx_apply_dss(e, iupd))) return r;
	} else {
		if ((r = surface_copy(e, iinit, iupd)) || (r = surface_zero(e, iwork))) return r;     // CopyData :2663, ZeroData :2693
		// Experiment (TMX_HVIS_PULL=1, judge's "node-unique" go / no-go): the DSS between the two passes is not run as a pass
		// of its own, the second pass averages the first pass's Laplacians while it loads them (k_hypervis<PULL>); on several
		// ranks the raw Laplacians of the rank boundary still travel, and the second pass starts once they have arrived.
		// Bit-identical, but a NO-GO: at ne30 L30 the second pass takes 166 instead of 67 us and moves 703 instead of 308 MB (every
		// seam node gathers its one to three partner values per field from other elements' rows: n^2 instead of n loads per
		// group, 8 bytes per lane from up to 30 different cache lines per wavefront instruction, not L2 hits) against the 62 us
		// and 248 MB of the DSS pass it replaces (profiles/r03_dss_pull_ab.txt).  Without tracers only (k_hypervis_tracers has no such form).
		const bool pull = TMX_EXP && e->hvis_pull && e->nt == 0 && work_is_scratch;      // (experiments flavour only)
		if (stage_can_split(e) && !e->sw) {
			// each pass boundary tiles first, its exchange overlapped with the interior tiles
			if ((r = produce_and_average(e, iwork, TMX_K_HYPERVIS, "hypervis pass (split)",
				[&](const KParams & q) { hvis_laplacians(e, q, inst(e, iinit), inst(e, iwork)); return TMX_OK; }, no_tail, !pull))) return r;
			if ((r = produce_and_average(e, iupd, TMX_K_HYPERVIS, "hypervis pass (split)",
				[&](const KParams & q) { hvis_apply(e, q, inst(e, iwork), inst(e, iinit), inst(e, iupd), dt, pull); return TMX_OK; }, no_tail))) return r;
		}
#if TMX_EXP
		else if (e->hvis_block && e->nt == 0 && !e->sw && e->n_hvblocks > 0) {
			// both passes fused with the DSS of the seams inside a patch (k_hypervis_block); k_dss only for the groups that span patches
			const int scale = (c.reference_length != 0.0) ? 1 : 0;
			for (int pass = 0; pass < 2; pass++) {
				const int idst = pass ? iupd : iwork;
				{
					ProfScope ps(e, TMX_K_HYPERVIS);
					if (pass == 0) tmxk_hypervis_block(e, p, inst(e, iinit), nullptr, inst(e, iwork), 1.0, 1.0, 1.0, 1.0, 0);
					else tmxk_hypervis_block(e, p, inst(e, iwork), inst(e, iinit), inst(e, iupd), -dt, c.nu_scalar, c.nu_div, c.nu_vort, scale);
				}
				if ((r = launch_check("hypervis pass (fused with the in-patch DSS)"))) return r;
				bool overlapped = false;
				if ((r = exchange(e, p, inst(e, idst), &overlapped))) return r;
				if ((r = dss_after_exchange(e, p, idst, overlapped, e->ngroups_inpatch))) return r;
			}
		}
#endif
		else {
			{ ProfScope ps(e, TMX_K_HYPERVIS); hvis_laplacians(e, p, inst(e, iinit), inst(e, iwork)); }
			if ((r = launch_check("hypervis pass 1"))) return r;
			if (pull) {
				bool overlapped = false;
				if ((r = exchange(e, p, inst(e, iwork), &overlapped))) return r;
				if (overlapped) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_recv, 0));
			} else if ((r = tmx_apply_dss(e, iwork))) return r;
			{ ProfScope ps(e, TMX_K_HYPERVIS); hvis_apply(e, p, inst(e, iwork), inst(e, iinit), inst(e, iupd), dt, pull); }
			if ((r = launch_check("hypervis pass 2"))) return r;
			if ((r = tmx_apply_dss(e, iupd))) return r;
		}
	}
	// APPLY_RAYLEIGH_WITH_HYPERVIS (Defines.h:70; HorizontalDynamicsFEM.cpp:2719-2724)
	if (e->rayleigh) {
		ProfScope ps(e, TMX_K_HYPERVIS);
		tmxk_rayleigh(e, p, inst(e, iupd), dt);
		return launch_check("rayleigh friction");
	}
	return TMX_OK;
}

// HorizontalDynamics::GetSubStepAfterSubCycleCount / SubStepAfterSubCycle (HorizontalDynamicsFEM.cpp:2574-2633): the two
// halves of the hyperviscosity step WITHOUT the DSS calls -- the caller (Model::SubStep, Model.cpp:286-) exchanges
// between them.  Sub-step 0: working <- Laplacians of initial; sub-step 1: update <- initial - dt nu Laplacians of
// working, tracer filter, Rayleigh friction.  *result receives the instance that holds the sub-step's output.
extern "C" int tmx_h_substep_after_subcycle_count(tmx_engine * e) {
	if (!e) return -1;
	return e->cfg.hypervis_order / 2;
}

extern "C" int tmx_h_substep_after_subcycle(tmx_engine * e, int iinit, int iupd, int iwork, double dt, int isubstep, int * result) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, iinit)) || (r = check_inst(e, iupd)) || (r = check_inst(e, iwork))) return r;
	REQUIRE(!e->sw, TMX_ERR_UNSUPPORTED, "SubStepAfterSubCycle with the shallow-water equation set is not supported");
	REQUIRE(isubstep == 0 || isubstep == 1, TMX_ERR_INVALID, "Invalid iSubStep %d", isubstep);
	REQUIRE(iinit != iwork && iupd != iwork, TMX_ERR_INVALID, "SubStepAfterSubCycle: working data must be distinct from initial and update data");
	KParams p = make_params(e);
	ProfScope ps(e, TMX_K_HYPERVIS);
	if (isubstep == 0) {
		hvis_laplacians(e, p, inst(e, iinit), inst(e, iwork));
		if (result) *result = iwork;
		return launch_check("hypervis sub-step 0");
	}
	REQUIRE(iinit != iupd, TMX_ERR_INVALID, "SubStepAfterSubCycle: initial and update data must be distinct");
	hvis_apply(e, p, inst(e, iwork), inst(e, iinit), inst(e, iupd), dt);
	if (e->rayleigh) tmxk_rayleigh(e, p, inst(e, iupd), dt);
	if (result) *result = iupd;
	return launch_check("hypervis sub-step 1");
}

bool hypervis_active(const tmx_engine * e) {
	const tmx_config & c = e->cfg;
	return !((c.nu_scalar == 0.0 && c.nu_div == 0.0 && c.nu_vort == 0.0) || c.hypervis_order == 0);
}


extern "C" int tmx_v_step_implicit_terms_explicitly(tmx_engine * e, int iinit, int iupd, double dt) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, iinit)) || (r = check_inst(e, iupd))) return r;
	REQUIRE(iinit != iupd && dt != 0.0, TMX_ERR_INVALID, "StepImplicitTermsExplicitly: distinct instances and non-zero dt required");
	if (e->sw) return TMX_OK;      // VerticalDynamicsStub inherits the empty VerticalDynamics::StepImplicitTermsExplicitly (VerticalDynamics.h:89-95)
	if (e->fully_explicit && (r = check_reference_state(e))) return r;
	// refusal before the first kernel (the terms kernel rewrites the update instance; the tracer update follows it): the instance stays as it is
	if ((r = tmx_vertical_fit(e, e->fully_explicit ? TMX_FIT_VT_EXPLICIT : TMX_FIT_VT_ALL))) return r;
	ProfScope ps(e, TMX_K_VI_ASSEMBLE);
	tmxk_vi_terms_explicit(e, make_params(e), inst(e, iinit), inst(e, iupd), dt, false);
	if (e->nt > 0) {
		// UpdateColumnTracers(dt, initial, update, ...) of every column, :600-608; in the fully explicit mode it takes its explicit branch
		// here as everywhere (:3912, :4048: diagonal matrix, xi_dot of the initial column, uniform diffusion of the mixing ratio)
		const int rt = e->fully_explicit ? tmxk_vi_tracers_explicit(e, make_params(e), inst(e, iinit), inst(e, iupd), dt)
			: tmxk_vi_tracers_all(e, make_params(e), inst(e, iinit), inst(e, iupd), dt);
		REQUIRE(rt == 0, TMX_ERR_UNSUPPORTED, "tracer column update: %d levels do not fit the LDS working set", e->L);
	}
	return launch_check("v_step_implicit_terms_explicitly");
}
// ---------------------------------------------------------------------------------------------
// output interpolation (Grid::ReduceInterpolate)

struct tmx_interp {
	tmx_engine * owner = nullptr;
	int npts = 0, nreta = 0;
	bool has_rll = false;
	int * d_col0 = nullptr;
	double * d_ca = nullptr, * d_cb = nullptr, * d_rll = nullptr, * d_opn = nullptr, * d_ope = nullptr, * d_out = nullptr;
	size_t out_n = 0;
};

// plans outlive their engine safely: tmx_destroy clears `owner` of every plan the engine still lists
void interp_orphan(tmx_engine * e) {
	for (tmx_interp * q : e->interps) q->owner = nullptr;
	e->interps.clear();
}

extern "C" void tmx_interp_destroy(tmx_interp * q) {
	if (!q) return;
	if (q->owner) {
		if (q->owner->stream) hipStreamSynchronize(q->owner->stream);
		auto & v = q->owner->interps;
		v.erase(std::remove(v.begin(), v.end(), q), v.end());
	}
	hipFree(q->d_col0); hipFree(q->d_ca); hipFree(q->d_cb); hipFree(q->d_rll); hipFree(q->d_opn); hipFree(q->d_ope); hipFree(q->d_out);
	delete q;
}

extern "C" int tmx_interp_create(tmx_engine * e, const tmx_interp_points * pts, tmx_interp ** out) {
	int r; if ((r = check_ready(e))) return r;
	REQUIRE(pts && out, TMX_ERR_INVALID, "tmx_interp_create: null argument");
	REQUIRE(!e->sw, TMX_ERR_UNSUPPORTED, "output interpolation with the shallow-water equation set is not supported");
	REQUIRE(pts->n_points > 0 && pts->n_reta > 0 && pts->patch && pts->node_a && pts->node_b && pts->coeff_a && pts->coeff_b &&
		pts->op_levels && pts->op_interfaces, TMX_ERR_INVALID, "tmx_interp_create: incomplete point description");
	const int n = pts->n_points, L = e->L;
	std::vector<int> col0(n, -1);
	for (int i = 0; i < n; i++) {
		const int pi = pts->patch[i];
		REQUIRE(pi >= 0 && pi < e->cfg.n_patches, TMX_ERR_INVALID, "interpolation point %d: patch %d out of range", i, pi);
		const PatchInfo & P = e->patches[pi];
		if (P.owner != e->cfg.rank) continue;
		const int a = pts->node_a[i], b = pts->node_b[i];
		REQUIRE(a >= 1 && b >= 1 && a + TMX_NP <= P.na - 1 && b + TMX_NP <= P.nb - 1 && (a - 1) % TMX_NP == 0 && (b - 1) % TMX_NP == 0,
			TMX_ERR_INVALID, "interpolation point %d: (%d, %d) is not the first node of an element of patch %d", i, a, b, pi);
		col0[i] = col_of(P, a, b);
	}
	tmx_interp * q = new tmx_interp();
	q->owner = e; q->npts = n; q->nreta = pts->n_reta; q->has_rll = pts->rll_from_abp != nullptr;
	auto up = [&](auto ** d, const auto * hsrc, size_t cnt) -> bool {
		if (hipMalloc((void **)d, cnt * sizeof(**d)) != hipSuccess) return false;
		return hipMemcpy(*d, hsrc, cnt * sizeof(**d), hipMemcpyHostToDevice) == hipSuccess;
	};
	bool ok = up(&q->d_col0, col0.data(), (size_t)n) && up(&q->d_ca, pts->coeff_a, (size_t)n * 4) && up(&q->d_cb, pts->coeff_b, (size_t)n * 4) &&
		up(&q->d_opn, pts->op_levels, (size_t)pts->n_reta * L) && up(&q->d_ope, pts->op_interfaces, (size_t)pts->n_reta * (L + 1));
	if (ok && q->has_rll) ok = up(&q->d_rll, pts->rll_from_abp, (size_t)n * 4);
	q->out_n = (size_t)std::max(5, e->nt) * pts->n_reta * n;
	if (ok) ok = hipMalloc((void **)&q->d_out, q->out_n * sizeof(double)) == hipSuccess;
	if (!ok) { (void)hipGetLastError(); tmx_interp_destroy(q); tmx_set_error("tmx_interp_create: device allocation failed"); return TMX_ERR_DEVICE; }
	e->interps.push_back(q);
	*out = q;
	return TMX_OK;
}

static InterpArgs interp_args(const tmx_interp * q) {
	InterpArgs a;
	a.npts = q->npts; a.nreta = q->nreta; a.col0 = q->d_col0; a.ca = q->d_ca; a.cb = q->d_cb; a.rll = q->d_rll; a.opn = q->d_opn; a.ope = q->d_ope;
	return a;
}

extern "C" int tmx_interp_state(tmx_engine * e, tmx_interp * q, int instance, int only_at, int include_ref, int primitive,
	double earth_radius, double * out) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, instance, true))) return r;
	REQUIRE(q && q->owner == e && out, TMX_ERR_INVALID, "tmx_interp_state: bad plan / null output");
	REQUIRE(only_at >= 0 && only_at <= 2, TMX_ERR_INVALID, "tmx_interp_state: only_variables_at must be 0, 1 or 2");
	REQUIRE(!primitive || q->has_rll, TMX_ERR_INVALID, "tmx_interp_state: convert_to_primitive needs rll_from_abp in the plan");
	REQUIRE(!primitive || earth_radius > 0.0, TMX_ERR_INVALID, "tmx_interp_state: earth_radius must be positive");
	const double * xref = nullptr;
	if (!include_ref) {
		for (int lp : e->local_patches)
			REQUIRE(e->patches[lp].ref_set, TMX_ERR_INVALID, "tmx_interp_state without the reference state: tmx_set_patch_reference_state was not called for patch %d", lp);
		xref = e->d_ref;
	}
	tmxk_interp_state(e, make_params(e), interp_args(q), inst(e, instance), xref, only_at, primitive ? 1 : 0, earth_radius, q->d_out);
	if ((r = launch_check("interp_state"))) return r;
	HIPCHK(hipMemcpyAsync(out, q->d_out, (size_t)5 * q->nreta * q->npts * sizeof(double), hipMemcpyDeviceToHost, e->stream));
	HIPCHK(hipStreamSynchronize(e->stream));
	return TMX_OK;
}

extern "C" int tmx_interp_tracers(tmx_engine * e, tmx_interp * q, int instance, double * out) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, instance, true))) return r;
	REQUIRE(q && q->owner == e && out, TMX_ERR_INVALID, "tmx_interp_tracers: bad plan / null output");
	REQUIRE(e->nt > 0, TMX_ERR_INVALID, "Unable to Interpolate with no tracers.");
	tmxk_interp_tracers(e, make_params(e), interp_args(q), inst(e, instance), q->d_out);
	if ((r = launch_check("interp_tracers"))) return r;
	HIPCHK(hipMemcpyAsync(out, q->d_out, (size_t)e->nt * q->nreta * q->npts * sizeof(double), hipMemcpyDeviceToHost, e->stream));
	HIPCHK(hipStreamSynchronize(e->stream));
	return TMX_OK;
}

extern "C" int tmx_v_filter_negative_tracers(tmx_engine * e, int instance) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, instance))) return r;
	if (e->nt == 0) return TMX_OK;
	ProfScope ps(e, TMX_K_LINCOMB);
	tmxk_v_filter_tracers(e, make_params(e), inst(e, instance));
	return launch_check("v_filter_negative_tracers");
}

static int held_suarez_unique(tmx_engine * e, int instance, double dt, bool * done);
extern "C" int tmx_physics_held_suarez(tmx_engine * e, int instance, double dt) {
	int r; if ((r = check_ready(e))) return r;
	if (e->u.built && !e->sw) { bool done = false; if ((r = held_suarez_unique(e, instance, dt, &done)) || done) return r; }
	// The instance is node-unique but the forcing's inputs differ between the copies of a node (the reference's own latitude array does):
	// every stored copy is forced with its own inputs straight from the node-unique slabs -- the kernel's load is the conversion -- and the
	// instance is element-major afterwards; the next step's explicit stages read it copy by copy ("unique_mixed")
	{
		UniqueLayout & u = e->u;
		bool all_set = true;
		for (int lp : e->local_patches) all_set = all_set && e->patches[lp].physics_set;
		if (u.built && !e->sw && all_set && instance >= 0 && instance < e->cfg.n_instances && u.form[instance] == 1 && e->imap[instance] == instance && u.mixed_option) {
			bool shared = false;
			for (int b = 0; b < (int)e->imap.size(); b++) if (b != instance && (e->imap[b] == instance || e->uvmap[b] == instance)) shared = true;
			if (!shared) {
				if ((r = u_own_uv(e, instance))) return r;
				ProfScope ps(e, TMX_K_LINCOMB);
				tmxk_held_suarez(e, make_params(e), inst(e, instance), e->track_surface ? surface_slots(e, instance) : nullptr, dt,
					uinst(e, instance), (size_t)u.NUS, (const int *)u.d_ucol_of_dcol);
				u.form[instance] = 0; u.n_uform--; u.conversions++;
				return launch_check("physics_held_suarez (node-unique in, element-major out)");
			}
		}
	}
	if ((r = check_inst(e, instance))) return r;
	REQUIRE(!e->sw, TMX_ERR_UNSUPPORTED, "Held-Suarez physics with the shallow-water equation set is not supported");
	for (int lp : e->local_patches)
		REQUIRE(e->patches[lp].physics_set, TMX_ERR_INVALID, "tmx_set_patch_physics_inputs was not called for patch %d", lp);
	ProfScope ps(e, TMX_K_LINCOMB);
	tmxk_held_suarez(e, make_params(e), inst(e, instance), e->track_surface ? surface_slots(e, instance) : nullptr, dt);
	return launch_check("physics_held_suarez");
}
// the same on the unique columns of an instance that tmx_step left in node-unique form (no conversion there and back): the forcing is
// column by column, so with inputs that agree on all copies of a node (checked) one evaluation per node is every copy's result.
// *done = false: not applicable, the caller takes the element-major route.
static int held_suarez_unique(tmx_engine * e, int instance, double dt, bool * done) {
	*done = false;
	UniqueLayout & u = e->u;
	if (!u.built || instance < 0 || instance >= e->cfg.n_instances || u.form[instance] == 0 || e->imap[instance] != instance) return TMX_OK;
	for (int lp : e->local_patches) if (!e->patches[lp].physics_set) return TMX_OK;      // (the element-major route reports it)
	bool ok = false;
	int r = tmxu_physics_inputs(e, &ok);
	if (r || !ok) return r;
	if ((r = u_own_uv(e, instance))) return r;
	ProfScope ps(e, TMX_K_LINCOMB);
	// the tracked surface slots live with the element-major slot (the stage algebra of tmx_step keeps them there); their copies agree
	// whenever the instance's do (they are covered by the check that admitted the instance to the node-unique form)
	if (e->track_surface) tmxuk_gather_rows(e, 2, surface_slots(e, instance), u.d_surf_u);
	tmxk_held_suarez(e, tmxu_params_columns(e, make_params(e)), uinst(e, instance), e->track_surface ? u.d_surf_u : nullptr, dt);
	u.form[instance] = 1;      // (an element-major copy kept for a reader is stale now)
	u_written(e, instance);
	*done = true;
	return launch_check("physics_held_suarez (node-unique)");
}

// ---- Kessler microphysics (BASELINE config 4) ----
extern "C" int tmx_set_patch_level_heights(tmx_engine * e, int patch, const double * z_levels) {
	REQUIRE(e && z_levels, TMX_ERR_INVALID, "tmx_set_patch_level_heights: null argument");
	REQUIRE(patch >= 0 && patch < e->cfg.n_patches, TMX_ERR_INVALID, "patch index out of range");
	REQUIRE(!e->sw, TMX_ERR_UNSUPPORTED, "column physics with the shallow-water equation set is not supported");
	int r = ensure_layout(e);
	if (r) return r;
	PatchInfo & P = e->patches[patch];
	REQUIRE(P.owner == e->cfg.rank, TMX_ERR_INVALID, "patch %d is not owned by rank %d", patch, e->cfg.rank);
	const int L = e->L;
	const size_t NS = e->NS;
	if (e->h_zlev.empty()) e->h_zlev.assign((size_t)L * NS, 0.0);
	for (int i = 1; i < P.na - 1; i++)
	for (int j = 1; j < P.nb - 1; j++) {
		const int c = col_of(P, i, j);
		for (int k = 0; k < L; k++) e->h_zlev[(size_t)k * NS + c] = z_levels[((size_t)i * P.nb + j) * L + k];
	}
	P.zlev_set = true; e->zlev_dirty = true;
	return TMX_OK;
}

// level heights and the precipitation accumulator of the column physics (Kessler, DCMIP2016), allocated at first use; uploads changed heights
int column_physics_levels(tmx_engine * e) {
	const size_t NS = e->NS; const int L = e->L;
	if (!e->d_zlev) {
		HIPCHK(hipMalloc((void **)&e->d_zlev, (size_t)L * NS * sizeof(double)));
		HIPCHK(hipMalloc((void **)&e->d_prect, NS * sizeof(double)));
		HIPCHK(hipMemset(e->d_prect, 0, NS * sizeof(double)));
		e->hbm_bytes += (size_t)(L + 1) * NS * sizeof(double);
	}
	if (e->zlev_dirty) {
		HIPCHK(hipStreamSynchronize(e->stream));
		HIPCHK(hipMemcpy(e->d_zlev, e->h_zlev.data(), (size_t)L * NS * sizeof(double), hipMemcpyHostToDevice));
		e->zlev_dirty = false;
	}
	return TMX_OK;
}

extern "C" int tmx_physics_kessler(tmx_engine * e, int instance, double dt) {
	int r; if ((r = check_ready(e)) || (r = check_inst(e, instance))) return r;
	REQUIRE(!e->sw, TMX_ERR_UNSUPPORTED, "Kessler physics with the shallow-water equation set is not supported");
	REQUIRE(e->nt >= 3, TMX_ERR_INVALID, "Kessler physics needs the tracers RhoQv, RhoQc, RhoQr (n_tracers >= 3)");
	REQUIRE(dt > 0.0, TMX_ERR_INVALID, "tmx_physics_kessler: dt must be positive");
	for (int lp : e->local_patches)
		REQUIRE(e->patches[lp].zlev_set, TMX_ERR_INVALID, "tmx_set_patch_level_heights was not called for patch %d", lp);
	const size_t NS = e->NS; const int L = e->L;
	if ((r = column_physics_levels(e))) return r;
	if (!e->d_kes) {
		HIPCHK(hipMalloc((void **)&e->d_kes, (size_t)TMX_KES_NW * L * NS * sizeof(double)));
		e->hbm_bytes += (size_t)TMX_KES_NW * L * NS * sizeof(double);
	}
	ProfScope ps(e, TMX_K_LINCOMB);
	tmxk_kessler(e, make_params(e), inst(e, instance), dt);
	return launch_check("physics_kessler");
}

extern "C" int tmx_download_precipitation(tmx_engine * e, int patch, double * prect, int reset) {
	int r; if ((r = check_ready(e))) return r;
	REQUIRE(prect, TMX_ERR_INVALID, "tmx_download_precipitation: null argument");
	REQUIRE(patch >= 0 && patch < e->cfg.n_patches, TMX_ERR_INVALID, "patch index out of range");
	PatchInfo & P = e->patches[patch];
	REQUIRE(P.owner == e->cfg.rank, TMX_ERR_INVALID, "patch %d is not owned by rank %d", patch, e->cfg.rank);
	std::vector<double> v((size_t)P.nea * P.neb * TMX_NQ, 0.0);
	const int c0 = P.elem_base * TMX_NQ;
	if (e->d_prect) {
		HIPCHK(hipStreamSynchronize(e->stream));
		HIPCHK(hipMemcpy(v.data(), e->d_prect + c0, v.size() * sizeof(double), hipMemcpyDeviceToHost));
		if (reset) HIPCHK(hipMemset(e->d_prect + c0, 0, v.size() * sizeof(double)));
	}
	for (int i = 1; i < P.na - 1; i++)
	for (int j = 1; j < P.nb - 1; j++) prect[(size_t)i * P.nb + j] = v[col_of(P, i, j) - c0];
	return TMX_OK;
}

extern "C" int tmx_sync(tmx_engine * e) {
	int r; if ((r = check_ready(e))) return r;
	HIPCHK(hipStreamSynchronize(e->stream));
	prof_collect(e);
	int flag = 0;
	HIPCHK(hipMemcpy(&flag, e->d_flag, sizeof(int), hipMemcpyDeviceToHost));
	if (flag) HIPCHK(hipMemset(e->d_flag, 0, sizeof(int)));
	if (flag & TMX_FLAG_COMM) {
		// (a singular matrix reported in the same interval is a consequence: the columns were solved on stale ghost data)
		tmx_set_error("halo exchange: a neighbour rank's message did not arrive within the time-out (TMX_P2P_TIMEOUT_S = %d s) (peer-to-peer transport); "
			"the state of this engine is no longer valid: upload it again after tmx_halo_p2p_reset on every rank", e->p2p_timeout_s);
		return TMX_ERR_COMM;
	}
	if (flag & TMX_FLAG_SINGULAR) {
		tmx_set_error("column solve failed: exactly singular band matrix (LAPACK dgbsv info > 0)");
		return TMX_ERR_SINGULAR;
	}
	return TMX_OK;
}

