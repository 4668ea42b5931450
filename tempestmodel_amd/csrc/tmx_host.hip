// tmx_host.hip -- host side of the engine, part 1: C ABI set-up (life cycle, operators, patches), state transfer, restart image, communicator
// and peer-to-peer set-up, introspection.  Part 2: tmx_step.hip; part 3: tmx_program.hip; tmx_finalize and its plan: tmx_plan.hip; the options: tmx_options.hip.
#include "tmx_hostshared.h"

// ---------------------------------------------------------------------------------------------
// errors

static thread_local std::string g_err;

void tmx_set_error(const char * fmt, ...) {
	char buf[1024];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	g_err = buf;
}

extern "C" const char * tmx_last_error(void) { return g_err.c_str(); }



// ---------------------------------------------------------------------------------------------
// RCCL, resolved at run time so the library loads without it (single-GPU use, CPU symbol checks)

NcclApi g_nccl;

int load_rccl() {
	if (g_nccl.Send) return TMX_OK;
	// prefer an RCCL already in the process (torch ships its own); otherwise the ROCm one
	void * h = dlopen(nullptr, RTLD_NOW | RTLD_GLOBAL);
	if (!h || !dlsym(h, "ncclSend")) {
		const char * names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", nullptr };   // soname first: reuses an RCCL already loaded (torch bundles one)
		h = nullptr;
		for (int i = 0; names[i] && !h; i++) h = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
	}
	REQUIRE(h != nullptr, TMX_ERR_COMM, "RCCL not found (librccl.so)");
	g_nccl.lib = h;
	g_nccl.GetUniqueId = (fn_ncclGetUniqueId)dlsym(h, "ncclGetUniqueId");
	g_nccl.CommInitRank = (fn_ncclCommInitRank)dlsym(h, "ncclCommInitRank");
	g_nccl.CommDestroy = (fn_ncclCommDestroy)dlsym(h, "ncclCommDestroy");
	g_nccl.GroupStart = (fn_ncclGroupStart)dlsym(h, "ncclGroupStart");
	g_nccl.GroupEnd = (fn_ncclGroupEnd)dlsym(h, "ncclGroupEnd");
	g_nccl.Send = (fn_ncclSend)dlsym(h, "ncclSend");
	g_nccl.Recv = (fn_ncclRecv)dlsym(h, "ncclRecv");
	g_nccl.GetErrorString = (fn_ncclGetErrorString)dlsym(h, "ncclGetErrorString");
	g_nccl.CommCount = (fn_ncclCommCount)dlsym(h, "ncclCommCount");
	REQUIRE(g_nccl.GetUniqueId && g_nccl.CommInitRank && g_nccl.Send && g_nccl.Recv && g_nccl.GroupStart && g_nccl.GroupEnd,
		TMX_ERR_COMM, "RCCL symbols missing");
	return TMX_OK;
}

void prof_collect(tmx_engine * e) {
	for (auto & pe : e->prof_pending) {
		float ms = 0.f;
		hipEventSynchronize(pe.second.second);
		hipEventElapsedTime(&ms, pe.second.first, pe.second.second);
		e->prof_slots[pe.first].ms += ms;
		e->prof_slots[pe.first].n += 1;
		hipEventDestroy(pe.second.first);
		hipEventDestroy(pe.second.second);
	}
	e->prof_pending.clear();
}

// ---------------------------------------------------------------------------------------------
// life cycle

extern "C" int tmx_create(const tmx_config * cfg, tmx_engine ** out) {
	REQUIRE(cfg && out, TMX_ERR_INVALID, "tmx_create: null argument");
	REQUIRE(cfg->abi_version == TMX_ABI_VERSION, TMX_ERR_INVALID, "tmx_create: ABI version %d, library is %d", cfg->abi_version, TMX_ABI_VERSION);
	REQUIRE(cfg->horizontal_order == TMX_NP, TMX_ERR_UNSUPPORTED, "horizontal order %d unsupported (np = 4 only)", cfg->horizontal_order);
	REQUIRE(cfg->vertical_order == 1, TMX_ERR_UNSUPPORTED, "vertical order %d unsupported (1 only)", cfg->vertical_order);
	REQUIRE(cfg->n_tracers >= 0 && cfg->n_tracers <= 16, TMX_ERR_UNSUPPORTED, "0..16 tracers supported, got %d", cfg->n_tracers);
	REQUIRE(cfg->n_tracers == 0 || cfg->equation_set == TMX_EQN_PRIMITIVE_NONHYDROSTATIC, TMX_ERR_UNSUPPORTED, "tracers are supported with the nonhydrostatic equation set only");
	REQUIRE(cfg->hypervis_order == 4 || cfg->hypervis_order == 2 || cfg->hypervis_order == 0, TMX_ERR_UNSUPPORTED, "hyperviscosity order %d unsupported (0, 2 or 4)", cfg->hypervis_order);
	REQUIRE((cfg->fully_explicit == 0 || cfg->fully_explicit == 1) && (cfg->uniform_diffusion == 0 || cfg->uniform_diffusion == 1), TMX_ERR_INVALID, "fully_explicit / uniform_diffusion must be 0 or 1");
	REQUIRE(!(cfg->fully_explicit || cfg->uniform_diffusion) || cfg->equation_set == TMX_EQN_PRIMITIVE_NONHYDROSTATIC, TMX_ERR_UNSUPPORTED,
		"fully explicit vertical dynamics / uniform diffusion need the nonhydrostatic equation set");
	// With implicit vertical dynamics the reference's StepExplicit diffuses whatever column the previous StepImplicit
	// left in m_dStateNode (SetupReferenceColumn is not called there, VerticalDynamicsFEM.cpp:745-812 vs :1059-1105)
	// and its tracer update throws "Not implemented" (:3914-3917): no stock case uses that combination.
	REQUIRE(!cfg->uniform_diffusion || cfg->fully_explicit, TMX_ERR_UNSUPPORTED, "uniform diffusion is supported with fully explicit vertical dynamics only (the supercell configuration)");
	REQUIRE(!cfg->uniform_diffusion || cfg->ztop > 0.0, TMX_ERR_INVALID, "uniform diffusion needs cfg.ztop > 0");
	REQUIRE(cfg->equation_set == TMX_EQN_PRIMITIVE_NONHYDROSTATIC || cfg->equation_set == TMX_EQN_SHALLOW_WATER,
		TMX_ERR_UNSUPPORTED, "equation set %d unsupported", cfg->equation_set);
	if (cfg->equation_set == TMX_EQN_SHALLOW_WATER) REQUIRE(cfg->levels == 1, TMX_ERR_INVALID, "shallow water needs levels == 1");
	else REQUIRE(cfg->levels >= 3, TMX_ERR_INVALID, "levels must be >= 3");
	REQUIRE(cfg->n_patches >= 1 && cfg->n_instances >= 1, TMX_ERR_INVALID, "bad patch / instance count");
	REQUIRE(cfg->n_instances <= 32, TMX_ERR_UNSUPPORTED, "%d data instances: the stepper programs track instances in 32-bit masks", cfg->n_instances);
	REQUIRE(cfg->n_ranks >= 1 && cfg->rank >= 0 && cfg->rank < cfg->n_ranks, TMX_ERR_INVALID, "bad rank %d of %d", cfg->rank, cfg->n_ranks);
	tmx_engine * e = new tmx_engine();
	e->cfg = *cfg;
	e->L = cfg->levels;
	e->patches.resize(cfg->n_patches);
	e->nt = cfg->n_tracers;
	e->nslab = 5 * e->L + 1 + e->nt * e->L;
	e->sw = (cfg->equation_set == TMX_EQN_SHALLOW_WATER);
	e->fully_explicit = cfg->fully_explicit != 0; e->udiff = cfg->uniform_diffusion != 0;
	e->imap.resize(cfg->n_instances);
	for (int k = 0; k < cfg->n_instances; k++) e->imap[k] = k;
	e->uvmap = e->imap;
	if (e->sw) { e->h_ops.assign((size_t)TMX_OP_COUNT * (e->L + 1) * TMX_OPW, 0.0); e->ops_set = true;
		for (int i = 0; i < 16; i++) { e->h_dx[i] = 0.0; e->h_stiff[i] = 0.0; } }
	// (no environment variable is read here: options arrive through tmx_set_option, or -- for test and bench plumbing that wants the
	// old TMX_* variables -- through an explicit tmx_options_from_environment call, which reports what it applied)
	if (!plan_only(e)) {
		int ndev = 0;
		hipError_t r = hipGetDeviceCount(&ndev);
		if (r != hipSuccess || ndev == 0) {
			delete e;
			tmx_set_error("tmx_create: no HIP device available (%s); this engine has no CPU path", hipGetErrorString(r));
			return TMX_ERR_DEVICE;
		}
		if (r == hipSuccess && cfg->device >= 0) r = hipSetDevice(cfg->device);
		if (r == hipSuccess) r = hipGetDevice(&e->device);
		if (r == hipSuccess) r = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
		if (r != hipSuccess) {
			delete e;
			tmx_set_error("tmx_create: device %d: %s", cfg->device, hipGetErrorString(r));
			return TMX_ERR_DEVICE;
		}
	}
	*out = e;
	return TMX_OK;
}

static void free_dev(void * p) { if (p) hipFree(p); }
extern "C" void tmx_destroy(tmx_engine * e) {
	if (!e) return;
	interp_orphan(e);
	if (!plan_only(e)) {
		if (e->stream) hipStreamSynchronize(e->stream);
		for (auto & g : e->graphs) hipGraphExecDestroy(g.exec);
		if (e->h_stage) hipHostFree(e->h_stage);
		if (e->xstream) { hipStreamSynchronize(e->xstream); hipStreamDestroy(e->xstream); hipEventDestroy(e->ev_pack); hipEventDestroy(e->ev_recv); }
		prof_collect(e);
		if (e->comm && g_nccl.CommDestroy) g_nccl.CommDestroy(e->comm);
		free_dev(e->d_state); free_dev(e->d_ref); free_dev(e->d_refd); free_dev(e->d_area); free_dev(e->d_w0); free_dev(e->d_eta); free_dev(e->d_ray_nu); free_dev(e->d_ray_ref); free_dev(e->d_g2d); free_dev(e->d_g3n); free_dev(e->d_g3e); free_dev(e->d_ops);
		free_dev(e->d_scratch); free_dev(e->d_grp_cols); free_dev(e->d_colref); free_dev(e->d_hvblocks); free_dev(e->d_grp_n); free_dev(e->d_grp_x); free_dev(e->d_grp_type); free_dev(e->d_xmat); free_dev(e->d_zlev); free_dev(e->d_prect); free_dev(e->d_kes); free_dev(e->d_dcmip); free_dev(e->d_zint); free_dev(e->d_dcw); free_dev(e->d_quads_early); free_dev(e->d_quads_late); free_dev(e->d_pivot_stats); free_dev(e->d_image);
		if (e->d_ghost_own) e->d_ghost = e->d_ghost_own;          // p2p mode pointed d_ghost into the shared block
		for (void * q : e->p2p_peer) if (q) hipIpcCloseMemHandle(q);
		free_dev(e->p2p_block); free_dev(e->d_p2p_dst); free_dev(e->d_p2p_flag); free_dev(e->d_send_peer); free_dev(e->d_send_within); free_dev(e->d_p2p_peers);
		free_dev(e->d_ghost); free_dev(e->d_sendbuf); free_dev(e->d_send_cols); free_dev(e->d_send_base); free_dev(e->d_send_stride); free_dev(e->d_ghost_base); free_dev(e->d_ghost_stride); free_dev(e->d_ucol); free_dev(e->d_udep);
		free_dev(e->d_ab); free_dev(e->d_rhs); free_dev(e->d_flag);
		tmxu_free(e);
		if (e->stream) hipStreamDestroy(e->stream);
	}
	delete e;
}

// ---------------------------------------------------------------------------------------------
// operators

extern "C" int tmx_set_operators(tmx_engine * e, const double * dx_basis, const double * stiffness,
	const double * const * coeff, const int * const * ix_begin, const int * const * ix_end,
	const int * n_out, const int * n_in)
{
	REQUIRE(e && dx_basis && stiffness, TMX_ERR_INVALID, "tmx_set_operators: null argument");
	REQUIRE(e->sw || (coeff && ix_begin && ix_end && n_out && n_in), TMX_ERR_INVALID, "tmx_set_operators: null argument");
	const int L = e->L;
	memcpy(e->h_dx, dx_basis, sizeof(double) * 16);
	memcpy(e->h_stiff, stiffness, sizeof(double) * 16);
	if (e->sw) { e->ops_set = true; return TMX_OK; }      // no column operators on one level
	// expected shapes (GridGLL.cpp:278-362)
	const int exp_out[TMX_OP_COUNT] = { L + 1, L, L, L + 1, L, L + 1, L, L + 1, L, L };
	const int exp_in[TMX_OP_COUNT]  = { L, L + 1, L, L, L + 1, L + 1, L, L + 1, L, L };
	// offsets each kernel is written for (vertical order 1 stencils)
	const int lo[TMX_OP_COUNT] = { -2, 0, -1, -1, 0, -1, -1, -1, 0, -1 };
	const int hi[TMX_OP_COUNT] = { 1, 1, 1, 0, 1, 1, 1, 1, 1, 0 };
	e->h_ops.assign((size_t)TMX_OP_COUNT * (L + 1) * TMX_OPW, 0.0);
	for (int op = 0; op < TMX_OP_COUNT; op++) {
		REQUIRE(n_out[op] == exp_out[op] && n_in[op] == exp_in[op], TMX_ERR_INVALID,
			"operator %d has shape %dx%d, expected %dx%d", op, n_out[op], n_in[op], exp_out[op], exp_in[op]);
		for (int k = 0; k < n_out[op]; k++) {
			for (int l = ix_begin[op][k]; l < ix_end[op][k]; l++) {
				const double c = coeff[op][(size_t)k * n_in[op] + l];
				if (c == 0.0) continue;
				const int off = l - k;
				REQUIRE(off >= lo[op] && off <= hi[op], TMX_ERR_UNSUPPORTED,
					"operator %d row %d has a coefficient at offset %d outside the vertical-order-1 stencil", op, k, off);
				if (op == TMX_OP_INTERP_NODE_TO_REDGE && k >= 1 && k <= L - 1)
					REQUIRE(off == -1 || off == 0, TMX_ERR_UNSUPPORTED, "interior row %d of InterpNodeToREdge is not a two-point stencil", k);
				e->h_ops[((size_t)op * (L + 1) + k) * TMX_OPW + (off + 2)] = c;
			}
		}
	}
	e->ops_set = true;
	return TMX_OK;
}

// ---------------------------------------------------------------------------------------------
// patches, halos, layout

extern "C" int tmx_define_patch(tmx_engine * e, int patch, int panel, int elems_a, int elems_b, int owner_rank,
	const int * neighbor_panels)
{
	REQUIRE(e && neighbor_panels, TMX_ERR_INVALID, "tmx_define_patch: null argument");
	REQUIRE(!e->finalized && e->ne_local == 0, TMX_ERR_INVALID, "tmx_define_patch after layout was fixed");
	REQUIRE(patch >= 0 && patch < e->cfg.n_patches, TMX_ERR_INVALID, "patch index %d out of range", patch);
	REQUIRE(elems_a > 0 && elems_b > 0 && panel >= 0 && panel < 6, TMX_ERR_INVALID, "bad patch box");
	REQUIRE(owner_rank >= 0 && owner_rank < e->cfg.n_ranks, TMX_ERR_INVALID, "owner rank %d out of range", owner_rank);
	PatchInfo & P = e->patches[patch];
	P.defined = true; P.panel = panel; P.nea = elems_a; P.neb = elems_b;
	P.na = TMX_NP * elems_a + 2; P.nb = TMX_NP * elems_b + 2; P.owner = owner_rank;
	memcpy(P.nbp, neighbor_panels, sizeof(int) * 8);
	return TMX_OK;
}

// GridPatchGLL::GetElementDeltaA / GetElementDeltaB of one patch.  The reference forms them as the difference of two
// element-edge coordinates of the patch (GridPatchGLL.cpp:67-75), so they differ from pi / (2 ne) -- and from patch to
// patch -- in the last bits, and every horizontal derivative is scaled with the patch's own 1 / delta (HorizontalDynamicsFEM.
// cpp:837-838, 1957-1958 ...).  Optional: without the call cfg.element_delta_a serves both directions of the patch.
extern "C" int tmx_set_patch_element_spacing(tmx_engine * e, int patch, double delta_a, double delta_b) {
	REQUIRE(e, TMX_ERR_INVALID, "tmx_set_patch_element_spacing: null engine");
	REQUIRE(patch >= 0 && patch < e->cfg.n_patches && e->patches[patch].defined, TMX_ERR_INVALID, "patch %d not defined", patch);
	REQUIRE(!e->finalized, TMX_ERR_INVALID, "tmx_set_patch_element_spacing after tmx_finalize");
	REQUIRE(delta_a > 0.0 && delta_b > 0.0, TMX_ERR_INVALID, "element spacing must be positive");
	e->patches[patch].da = delta_a; e->patches[patch].db = delta_b;
	return TMX_OK;
}

extern "C" int tmx_set_patch_halo(tmx_engine * e, int patch, int n, const int * halo_i, const int * halo_j,
	const int * src_patch, const int * src_i, const int * src_j, const int * src_panel, const double * trans)
{
	REQUIRE(e && halo_i && halo_j && src_patch && src_i && src_j && src_panel && trans, TMX_ERR_INVALID, "tmx_set_patch_halo: null argument");
	REQUIRE(patch >= 0 && patch < e->cfg.n_patches && e->patches[patch].defined, TMX_ERR_INVALID, "patch %d not defined", patch);
	REQUIRE(!e->finalized, TMX_ERR_INVALID, "tmx_set_patch_halo after tmx_finalize");
	PatchInfo & P = e->patches[patch];
	P.hi.assign(halo_i, halo_i + n); P.hj.assign(halo_j, halo_j + n);
	P.hsp.assign(src_patch, src_patch + n); P.hsi.assign(src_i, src_i + n); P.hsj.assign(src_j, src_j + n);
	P.hspanel.assign(src_panel, src_panel + n);
	P.htrans.assign(trans, trans + (size_t)4 * n);
	for (int m = 0; m < n; m++) {
		REQUIRE(P.hi[m] >= 0 && P.hi[m] < P.na && P.hj[m] >= 0 && P.hj[m] < P.nb, TMX_ERR_INVALID, "halo node out of range");
		REQUIRE(P.hsp[m] < e->cfg.n_patches, TMX_ERR_INVALID, "halo source patch out of range");
	}
	P.halo_set = true;
	return TMX_OK;
}

int ensure_layout(tmx_engine * e) {
	if (e->ne_local > 0) return TMX_OK;
	int ne = 0;
	e->local_patches.clear();
	for (int p = 0; p < e->cfg.n_patches; p++) {
		PatchInfo & P = e->patches[p];
		REQUIRE(P.defined, TMX_ERR_INVALID, "patch %d was never defined", p);
		if (P.owner == e->cfg.rank) { P.elem_base = ne; ne += P.nea * P.neb; e->local_patches.push_back(p); }
	}
	REQUIRE(ne > 0, TMX_ERR_INVALID, "rank %d owns no patch", e->cfg.rank);
	e->ne_local = ne;
	e->ncol = ne * TMX_NQ;
	e->NS = ((e->ncol + TMX_TILE - 1) / TMX_TILE) * TMX_TILE;
	// + 2 "surface slots" behind the exchanged slabs: the interface-level-0 entries of rho and rho*theta of the reference's
	// REdge array, which nothing but the stage algebra touches and HeldSuarezPhysics reads (see surface_copy below)
	e->inst_stride = (size_t)(e->nslab + 2) * e->NS;
	const size_t NS = e->NS; const int L = e->L;
	e->h_g2d.assign((size_t)G2_COUNT * NS, 0.0);
	e->h_g3n.assign((size_t)G3N_COUNT * L * NS, 0.0);
	e->h_g3e.assign((size_t)G3E_COUNT * (L + 1) * NS, 0.0);
	// benign values in the padding columns
	for (size_t c = e->ncol; c < NS; c++) { e->h_g2d[G2_J2D * NS + c] = 1.0; e->h_g2d[G2_JN * NS + c] = 1.0; e->h_g2d[G2_JE * NS + c] = 1.0; }
	return TMX_OK;
}

extern "C" int tmx_set_patch_geometry(tmx_engine * e, int patch, const tmx_patch_geometry * g) {
	REQUIRE(e && g, TMX_ERR_INVALID, "tmx_set_patch_geometry: null argument");
	REQUIRE(patch >= 0 && patch < e->cfg.n_patches, TMX_ERR_INVALID, "patch index out of range");
	REQUIRE(!e->finalized, TMX_ERR_INVALID, "tmx_set_patch_geometry after tmx_finalize");
	int r = ensure_layout(e);
	if (r) return r;
	PatchInfo & P = e->patches[patch];
	REQUIRE(P.owner == e->cfg.rank, TMX_ERR_INVALID, "patch %d is not owned by rank %d", patch, e->cfg.rank);
	const int L = e->L, nb = P.nb;
	const size_t NS = e->NS;
	for (int i = 1; i < P.na - 1; i++)
	for (int j = 1; j < P.nb - 1; j++) {
		const int c = col_of(P, i, j);
		const size_t ij = (size_t)i * nb + j;
		e->h_g2d[G2_J2D * NS + c] = g->jacobian2d[ij];
		e->h_g2d[G2_F * NS + c] = g->coriolis_f[ij];
		e->h_g2d[G2_C2A0 * NS + c] = g->contra_metric_2d_a[ij * 2 + 0];
		e->h_g2d[G2_C2A1 * NS + c] = g->contra_metric_2d_a[ij * 2 + 1];
		e->h_g2d[G2_C2B1 * NS + c] = g->contra_metric_2d_b[ij * 2 + 1];
		REQUIRE(g->contra_metric_2d_b[ij * 2 + 0] == g->contra_metric_2d_a[ij * 2 + 1], TMX_ERR_UNSUPPORTED, "2-D contravariant metric is not symmetric");
		e->h_g2d[G2_JN * NS + c] = g->jacobian[ij * L];
		if (e->nt > 0) {
			REQUIRE(g->element_area_node, TMX_ERR_INVALID, "tracers need tmx_patch_geometry.element_area_node (patch %d)", patch);
			if (e->h_area.empty()) e->h_area.assign((size_t)L * NS, 0.0);
			for (int k = 0; k < L; k++) e->h_area[(size_t)k * NS + c] = g->element_area_node[ij * L + k];
		}
		if (e->sw) {
			// 2-D equation set: only the 2-D metric, the (single-level) Jacobian and the topography are used
			e->h_g2d[G2_JE * NS + c] = g->jacobian[ij * L];
			e->h_g2d[G2_DRX * NS + c] = 1.0;
			e->h_g2d[G2_ZS * NS + c] = g->topography ? g->topography[ij] : 0.0;
			continue;
		}
		e->h_g2d[G2_JE * NS + c] = g->jacobian_redge[ij * (L + 1)];
		e->h_g2d[G2_DRX * NS + c] = g->deriv_r_node[(ij * L) * 3 + 2];
		for (int k = 0; k < L; k++) {
			const size_t o = (ij * L + k) * 3;
			// structure of the reference metric (GridPatchCSGLL.cpp:444-494): level-independent
			// Jacobian / d_xi R, horizontal block equal to the 2-D metric, symmetric cross terms
			REQUIRE(g->jacobian[ij * L + k] == g->jacobian[ij * L] &&
			        g->deriv_r_node[o + 2] == g->deriv_r_node[(ij * L) * 3 + 2] &&
			        g->contra_metric_a[o + 0] == g->contra_metric_2d_a[ij * 2 + 0] &&
			        g->contra_metric_a[o + 1] == g->contra_metric_2d_a[ij * 2 + 1] &&
			        g->contra_metric_b[o + 0] == g->contra_metric_2d_b[ij * 2 + 0] &&
			        g->contra_metric_b[o + 1] == g->contra_metric_2d_b[ij * 2 + 1] &&
			        g->contra_metric_xi[o + 0] == g->contra_metric_a[o + 2] &&
			        g->contra_metric_xi[o + 1] == g->contra_metric_b[o + 2],
			        TMX_ERR_UNSUPPORTED, "node metric of patch %d does not have the Gal-Chen structure the engine stores", patch);
			const size_t d = (size_t)k * NS + c, s3 = (size_t)L * NS;
			e->h_g3n[G3N_CA2 * s3 + d] = g->contra_metric_a[o + 2];
			e->h_g3n[G3N_CB2 * s3 + d] = g->contra_metric_b[o + 2];
			e->h_g3n[G3N_CX2 * s3 + d] = g->contra_metric_xi[o + 2];
			e->h_g3n[G3N_DRA * s3 + d] = g->deriv_r_node[o + 0];
			e->h_g3n[G3N_DRB * s3 + d] = g->deriv_r_node[o + 1];
		}
		for (int k = 0; k <= L; k++) {
			const size_t o = (ij * (L + 1) + k) * 3;
			REQUIRE(g->jacobian_redge[ij * (L + 1) + k] == g->jacobian_redge[ij * (L + 1)] &&
			        g->deriv_r_redge[o + 2] == g->deriv_r_node[(ij * L) * 3 + 2] &&
			        g->contra_metric_a_redge[o + 0] == g->contra_metric_2d_a[ij * 2 + 0] &&
			        g->contra_metric_a_redge[o + 1] == g->contra_metric_2d_a[ij * 2 + 1] &&
			        g->contra_metric_b_redge[o + 0] == g->contra_metric_2d_b[ij * 2 + 0] &&
			        g->contra_metric_b_redge[o + 1] == g->contra_metric_2d_b[ij * 2 + 1] &&
			        g->contra_metric_xi_redge[o + 0] == g->contra_metric_a_redge[o + 2] &&
			        g->contra_metric_xi_redge[o + 1] == g->contra_metric_b_redge[o + 2],
			        TMX_ERR_UNSUPPORTED, "interface metric of patch %d does not have the Gal-Chen structure the engine stores", patch);
			const size_t d = (size_t)k * NS + c, s3 = (size_t)(L + 1) * NS;
			e->h_g3e[G3E_CX0 * s3 + d] = g->contra_metric_xi_redge[o + 0];
			e->h_g3e[G3E_CX1 * s3 + d] = g->contra_metric_xi_redge[o + 1];
			e->h_g3e[G3E_CX2 * s3 + d] = g->contra_metric_xi_redge[o + 2];
		}
	}
	P.geom_set = true;
	return TMX_OK;
}

// Closed form of the 3-D metric (GridPatchCSGLL.cpp:370-568).  The factors are accepted only if they
// reproduce every stored value bit for bit, so the kernels' in-register evaluation cannot change results.
extern "C" int tmx_set_patch_metric_factors(tmx_engine * e, int patch, const double * x_node, const double * y_node,
	const double * topography_deriv, double earth_radius, const double * reta_levels, const double * reta_interfaces)
{
	REQUIRE(e && x_node && y_node && topography_deriv && reta_levels && reta_interfaces, TMX_ERR_INVALID, "tmx_set_patch_metric_factors: null argument");
	REQUIRE(patch >= 0 && patch < e->cfg.n_patches, TMX_ERR_INVALID, "patch index out of range");
	REQUIRE(!e->finalized, TMX_ERR_INVALID, "tmx_set_patch_metric_factors after tmx_finalize");
	PatchInfo & P = e->patches[patch];
	REQUIRE(P.geom_set, TMX_ERR_INVALID, "tmx_set_patch_metric_factors before tmx_set_patch_geometry (patch %d)", patch);
	P.metric_ok = false;
	if (e->sw) return TMX_OK;                 // 2-D equation set: there is no 3-D metric
	const int L = e->L, nb = P.nb;
	const size_t NS = e->NS;
	std::vector<double> eta(2 * L + 1);
	for (int k = 0; k < L; k++) eta[k] = 1.0 - reta_levels[k];
	for (int k = 0; k <= L; k++) eta[L + k] = 1.0 - reta_interfaces[k];
	if (e->h_eta.empty()) e->h_eta = eta;
	else if (memcmp(e->h_eta.data(), eta.data(), eta.size() * sizeof(double)) != 0) return TMX_OK;   // patches disagree
	const size_t s3n = (size_t)L * NS, s3e = (size_t)(L + 1) * NS;
	bool ok = true;
	for (int i = 1; i < P.na - 1 && ok; i++)
	for (int j = 1; j < P.nb - 1 && ok; j++) {
		const int c = col_of(P, i, j);
		const size_t ij = (size_t)i * nb + j;
		const double dX = x_node[i], dY = y_node[j];
		const double dDelta2 = (1.0 + dX * dX + dY * dY);
		const double sc = dDelta2 / (1.0 + dX * dX) / (1.0 + dY * dY) / (earth_radius * earth_radius);
		const double dxr = e->h_g2d[G2_DRX * NS + c];
		const double mp = -sc / dxr, ma = (1.0 + dY * dY), mb = dX * dY, mc = (1.0 + dX * dX);
		const double daz = topography_deriv[ij * 2 + 0], dbz = topography_deriv[ij * 2 + 1];
		const double idx = 1.0 / dxr, idx2 = 1.0 / (dxr * dxr);
		// the 2-D metric must come from the same factors
		ok = ok && e->h_g2d[G2_C2A0 * NS + c] == sc * ma && e->h_g2d[G2_C2A1 * NS + c] == sc * dX * dY &&
		     e->h_g2d[G2_C2B1 * NS + c] == sc * mc;
		for (int k = 0; k < 2 * L + 1 && ok; k++) {
			const double dar = eta[k] * daz, dbr = eta[k] * dbz;
			const double c0 = mp * (ma * dar + mb * dbr);
			const double c1 = mp * (mb * dar + mc * dbr);
			const double c2 = idx2 - idx * (c0 * dar + c1 * dbr);
			if (k < L) {
				const size_t d = (size_t)k * NS + c;
				ok = e->h_g3n[G3N_CA2 * s3n + d] == c0 && e->h_g3n[G3N_CB2 * s3n + d] == c1 && e->h_g3n[G3N_CX2 * s3n + d] == c2 &&
				     e->h_g3n[G3N_DRA * s3n + d] == dar && e->h_g3n[G3N_DRB * s3n + d] == dbr;
			} else {
				const size_t d = (size_t)(k - L) * NS + c;
				ok = e->h_g3e[G3E_CX0 * s3e + d] == c0 && e->h_g3e[G3E_CX1 * s3e + d] == c1 && e->h_g3e[G3E_CX2 * s3e + d] == c2;
			}
		}
		e->h_g2d[G2_MP * NS + c] = mp; e->h_g2d[G2_MA * NS + c] = ma; e->h_g2d[G2_MB * NS + c] = mb; e->h_g2d[G2_MC * NS + c] = mc;
		e->h_g2d[G2_DAZ * NS + c] = daz; e->h_g2d[G2_DBZ * NS + c] = dbz; e->h_g2d[G2_IDX * NS + c] = idx; e->h_g2d[G2_IDX2 * NS + c] = idx2;
	}
	P.metric_ok = ok;
	return TMX_OK;
}

// Column physics inputs (latitude, Held-Suarez surface pressure) into two 2-D slabs
extern "C" int tmx_set_patch_physics_inputs(tmx_engine * e, int patch, const double * latitude, const double * surface_pressure) {
	REQUIRE(e && latitude, TMX_ERR_INVALID, "tmx_set_patch_physics_inputs: null argument");
	// surface_pressure == NULL: the forcing forms it from the tracked surface slots, as the reference does (see surface_copy)
	REQUIRE(e->patches_with_physics == 0 || e->track_surface == (surface_pressure == nullptr), TMX_ERR_INVALID,
		"tmx_set_patch_physics_inputs: every patch must use the same surface-pressure mode");
	e->track_surface = (surface_pressure == nullptr);
	REQUIRE(patch >= 0 && patch < e->cfg.n_patches, TMX_ERR_INVALID, "patch index out of range");
	REQUIRE(!e->sw, TMX_ERR_UNSUPPORTED, "column physics with the shallow-water equation set is not supported");
	int r = ensure_layout(e);
	if (r) return r;
	PatchInfo & P = e->patches[patch];
	REQUIRE(P.owner == e->cfg.rank, TMX_ERR_INVALID, "patch %d is not owned by rank %d", patch, e->cfg.rank);
	const size_t NS = e->NS;
	std::vector<double> lat((size_t)P.nea * P.neb * TMX_NQ), ps(lat.size()), sl(lat.size()), cl(lat.size());
	const int c0 = P.elem_base * TMX_NQ;
	for (int i = 1; i < P.na - 1; i++)
	for (int j = 1; j < P.nb - 1; j++) {
		const int c = col_of(P, i, j);
		lat[c - c0] = latitude[(size_t)i * P.nb + j];
		ps[c - c0] = surface_pressure ? surface_pressure[(size_t)i * P.nb + j] : 0.0;
		sl[c - c0] = sin(lat[c - c0]); cl[c - c0] = cos(lat[c - c0]);      // host libm: the values the reference computes per call
		if (!e->finalized) { e->h_g2d[G2_LAT * NS + c] = lat[c - c0]; e->h_g2d[G2_PS * NS + c] = ps[c - c0];
			e->h_g2d[G2_SINLAT * NS + c] = sl[c - c0]; e->h_g2d[G2_COSLAT * NS + c] = cl[c - c0]; }
	}
	if (e->finalized && !plan_only(e)) {       // may be refreshed at any time (the caller owns the source arrays)
		HIPCHK(hipStreamSynchronize(e->stream));
		HIPCHK(hipMemcpy(e->d_g2d + G2_LAT * NS + c0, lat.data(), lat.size() * sizeof(double), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(e->d_g2d + G2_PS * NS + c0, ps.data(), ps.size() * sizeof(double), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(e->d_g2d + G2_SINLAT * NS + c0, sl.data(), sl.size() * sizeof(double), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(e->d_g2d + G2_COSLAT * NS + c0, cl.data(), cl.size() * sizeof(double), hipMemcpyHostToDevice));
	}
	if (!P.physics_set) e->patches_with_physics++;
	P.physics_set = true;
	e->u.physics_dirty = true;
	return TMX_OK;
}

// Rayleigh friction inputs (GridPatch::GetRayleighStrength / GetReferenceState), gathered into the device layout
extern "C" int tmx_set_patch_rayleigh(tmx_engine * e, int patch, const double * strength_node, const double * strength_redge,
	const double * ref_node, const double * ref_redge)
{
	REQUIRE(e && strength_node && strength_redge && ref_node && ref_redge, TMX_ERR_INVALID, "tmx_set_patch_rayleigh: null argument");
	REQUIRE(patch >= 0 && patch < e->cfg.n_patches, TMX_ERR_INVALID, "patch index out of range");
	REQUIRE(!e->finalized, TMX_ERR_INVALID, "tmx_set_patch_rayleigh after tmx_finalize");
	REQUIRE(!e->sw, TMX_ERR_UNSUPPORTED, "Rayleigh friction with the shallow-water equation set is not supported");
	int r = ensure_layout(e);
	if (r) return r;
	PatchInfo & P = e->patches[patch];
	REQUIRE(P.owner == e->cfg.rank, TMX_ERR_INVALID, "patch %d is not owned by rank %d", patch, e->cfg.rank);
	const int L = e->L, na = P.na, nb = P.nb;
	const size_t NS = e->NS;
	if (e->h_ray_nu.empty()) { e->h_ray_nu.assign((size_t)(2 * L + 1) * NS, 0.0); e->h_ray_ref.assign((size_t)(4 * L + 1) * NS, 0.0); }
	for (int i = 1; i < na - 1; i++)
	for (int j = 1; j < nb - 1; j++) {
		const int c = col_of(P, i, j);
		const size_t ij = (size_t)i * nb + j;
		for (int k = 0; k < L; k++) {
			e->h_ray_nu[(size_t)k * NS + c] = strength_node[ij * L + k];
			for (int v = 0; v < 3; v++)      // U, V, rho*theta
				e->h_ray_ref[(size_t)(v * L + k) * NS + c] = ref_node[(((size_t)v * na + i) * nb + j) * L + k];
		}
		for (int k = 0; k <= L; k++) {
			e->h_ray_nu[(size_t)(L + k) * NS + c] = strength_redge[ij * (L + 1) + k];
			e->h_ray_ref[(size_t)(3 * L + k) * NS + c] = ref_redge[(((size_t)3 * na + i) * nb + j) * (L + 1) + k];
		}
	}
	P.rayleigh_set = true;
	return TMX_OK;
}

// ---------------------------------------------------------------------------------------------
// state transfer

static int check_state_args(tmx_engine * e, int patch, int instance, bool read_only = false) {
	REQUIRE(e && e->finalized && !plan_only(e), TMX_ERR_INVALID, "engine not finalized");
	REQUIRE(patch >= 0 && patch < e->cfg.n_patches && e->patches[patch].owner == e->cfg.rank, TMX_ERR_INVALID, "patch %d is not local", patch);
	REQUIRE(instance >= 0 && instance < e->cfg.n_instances, TMX_ERR_INVALID, "instance %d out of range", instance);
	return settle_instance(e, instance, read_only);
}

// ---------------------------------------------------------------------------------------------
// Host <-> slab transposition at the ABI boundary.  The reference keeps a column contiguous ([var][i][j][k]); the
// device keeps a level contiguous over columns ([slab][column]).  The staging buffer is walked in tiles of 64
// device columns (= 4 elements: 64 x L doubles per variable stay in L1 while all levels of the tile are moved) and
// the tiles are dealt to a few host threads -- the naive column-at-a-time loop read one double per cache line
// (measured at ne30 L30: download 45 -> see DESIGN.md section 5).
static void host_parallel(int ntiles, const std::function<void(int, int)> & fn) {
	int nthr = (int)std::thread::hardware_concurrency();
	if (nthr > 8) nthr = 8;
	if (nthr < 1 || ntiles < 4 * nthr) { fn(0, ntiles); return; }
	std::vector<std::thread> th;
	const int per = (ntiles + nthr - 1) / nthr;
	for (int t = 0; t < nthr; t++) {
		const int a = t * per, b = std::min(ntiles, a + per);
		if (a < b) th.emplace_back(fn, a, b);
	}
	for (auto & x : th) x.join();
}

// pinned staging buffer of the engine (grown on demand): no per-call allocation / zero fill, DMA at full PCIe rate
static double * stage_buffer(tmx_engine * e, size_t n) {
	if (e->h_stage_n < n) {
		if (e->h_stage) hipHostFree(e->h_stage);
		e->h_stage = nullptr; e->h_stage_n = 0;
		if (hipHostMalloc((void **)&e->h_stage, n * sizeof(double), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		e->h_stage_n = n;
	}
	return e->h_stage;
}

// host node offset (i * nb + j) of every device column of the patch, device order
static const std::vector<int> & host_offsets(tmx_engine * e, int patch) {
	PatchInfo & P = e->patches[patch];
	if (P.hoff.empty()) {
		const int c0 = P.elem_base * TMX_NQ;
		P.hoff.assign((size_t)P.nea * P.neb * TMX_NQ, 0);
		for (int i = 1; i < P.na - 1; i++) for (int j = 1; j < P.nb - 1; j++) P.hoff[col_of(P, i, j) - c0] = i * P.nb + j;
	}
	return P.hoff;
}

// one variable: host[(var_off + hoff[c]) * nlev + k]  <->  buf[(slab0 + k) * ncp + c], columns [ca, cb)
static inline void xpose_to_buf(const double * host, size_t var_off, int nlev, double * buf, int slab0, int ncp, const int * hoff, int ca, int cb) {
	for (int k = 0; k < nlev; k++) {
		double * row = buf + (size_t)(slab0 + k) * ncp;
		for (int c = ca; c < cb; c++) row[c] = host[(var_off + hoff[c]) * nlev + k];
	}
}
static inline void xpose_to_host(double * host, size_t var_off, int nlev, const double * buf, int slab0, int ncp, const int * hoff, int ca, int cb) {
	for (int k = 0; k < nlev; k++) {
		const double * row = buf + (size_t)(slab0 + k) * ncp;
		for (int c = ca; c < cb; c++) host[(var_off + hoff[c]) * nlev + k] = row[c];
	}
}

// GridPatch::GetReferenceState / GetReferenceTracers -> the reference "instance" of the uniform diffusion
extern "C" int tmx_set_patch_reference_state(tmx_engine * e, int patch, const double * ref_node, const double * ref_redge, const double * ref_tracers) {
	int r = check_state_args(e, patch, 0);
	if (r) return r;
	if (!e->d_ref) {      // engines without uniform diffusion keep a reference state only if the caller provides one (tmx_interp_state)
		const size_t rb = (size_t)e->nslab * e->NS * sizeof(double);
		HIPCHK(hipMalloc((void **)&e->d_ref, rb)); HIPCHK(hipMemset(e->d_ref, 0, rb)); e->hbm_bytes += rb;
	}
	REQUIRE(ref_node && ref_redge && (ref_tracers || e->nt == 0), TMX_ERR_INVALID, "tmx_set_patch_reference_state: null array");
	PatchInfo & P = e->patches[patch];
	const int L = e->L, na = P.na, nb = P.nb;
	const int ncp = P.nea * P.neb * TMX_NQ, c0 = P.elem_base * TMX_NQ;
	std::vector<double> buf((size_t)e->nslab * ncp);
	const int nodevar[4] = { 0, 1, 2, 4 };
	for (int i = 1; i < na - 1; i++) for (int j = 1; j < nb - 1; j++) {
		const int c = col_of(P, i, j) - c0;
		for (int v = 0; v < 4; v++) for (int k = 0; k < L; k++)
			buf[(size_t)(v * L + k) * ncp + c] = ref_node[(((size_t)nodevar[v] * na + i) * nb + j) * L + k];
		for (int k = 0; k <= L; k++)
			buf[(size_t)(4 * L + k) * ncp + c] = ref_redge[(((size_t)3 * na + i) * nb + j) * (L + 1) + k];
		for (int v = 0; v < e->nt; v++) for (int k = 0; k < L; k++)
			buf[(size_t)TMX_SLAB_Q(L, v, k) * ncp + c] = ref_tracers[(((size_t)v * na + i) * nb + j) * L + k];
	}
	HIPCHK(hipStreamSynchronize(e->stream));
	HIPCHK(hipMemcpy2D(e->d_ref + c0, (size_t)e->NS * sizeof(double), buf.data(), (size_t)ncp * sizeof(double),
		(size_t)ncp * sizeof(double), e->nslab, hipMemcpyHostToDevice));
	P.ref_set = true;
	e->refd_valid = false;
	return TMX_OK;
}

int check_reference_state(tmx_engine * e) {
	if (!e->udiff) return TMX_OK;
	for (int lp : e->local_patches)
		REQUIRE(e->patches[lp].ref_set, TMX_ERR_INVALID, "uniform diffusion: tmx_set_patch_reference_state was not called for patch %d", lp);
	return TMX_OK;
}

extern "C" int tmx_upload_state(tmx_engine * e, int patch, int instance, const double * node, const double * redge) {
	int r = check_state_args(e, patch, instance);
	if (r) return r;
	REQUIRE(node && (redge || e->sw), TMX_ERR_INVALID, "tmx_upload_state: null array");
	const PatchInfo & P = e->patches[patch];
	const int L = e->L, na = P.na, nb = P.nb;
	const int ncp = P.nea * P.neb * TMX_NQ, c0 = P.elem_base * TMX_NQ;
	const int nstate = 5 * L + 1;          // state slabs; tracer slabs are moved by tmx_upload_tracers
	HIPCHK(hipStreamSynchronize(e->stream));      // the staging buffer may still feed an earlier copy
	double * bufp = stage_buffer(e, (size_t)nstate * ncp);
	REQUIRE(bufp, TMX_ERR_DEVICE, "cannot allocate the pinned staging buffer");
	struct { double * p; double * data() const { return p; } } buf = { bufp };
	const int nodevar[4] = { 0, 1, 2, 4 };
	const int * hoff = host_offsets(e, patch).data();
	const size_t nn = (size_t)na * nb;
	const bool sw = e->sw;
	host_parallel((ncp + 63) / 64, [&](int ta, int tb) {
		for (int t = ta; t < tb; t++) {
			const int ca = t * 64, cb = std::min(ncp, ca + 64);
			if (sw) {        // node is [3][na][nb][1]: U, V, H -> slabs U, V, "rho*theta"
				for (int v = 0; v < 3; v++) xpose_to_buf(node, (size_t)v * nn, 1, buf.data(), v, ncp, hoff, ca, cb);
				continue;
			}
			for (int v = 0; v < 4; v++) xpose_to_buf(node, (size_t)nodevar[v] * nn, L, buf.data(), v * L, ncp, hoff, ca, cb);
			xpose_to_buf(redge, (size_t)3 * nn, L + 1, buf.data(), 4 * L, ncp, hoff, ca, cb);
		}
	});
	HIPCHK(hipStreamSynchronize(e->stream));
	HIPCHK(hipMemcpy2D(e->d_state + (size_t)instance * e->inst_stride + c0, (size_t)e->NS * sizeof(double),
		buf.data(), (size_t)ncp * sizeof(double), (size_t)ncp * sizeof(double), nstate, hipMemcpyHostToDevice));
	if (!sw) {
		// surface slots: interface-level-0 entries of rho (REdge component 4) and rho*theta (component 2), see surface_copy
		std::vector<double> ss((size_t)2 * ncp);
		for (int c = 0; c < ncp; c++) {
			ss[c] = redge[((size_t)4 * nn + hoff[c]) * (L + 1)];
			ss[(size_t)ncp + c] = redge[((size_t)2 * nn + hoff[c]) * (L + 1)];
		}
		HIPCHK(hipMemcpy2D(e->d_state + (size_t)instance * e->inst_stride + (size_t)e->nslab * e->NS + c0, (size_t)e->NS * sizeof(double),
			ss.data(), (size_t)ncp * sizeof(double), (size_t)ncp * sizeof(double), 2, hipMemcpyHostToDevice));
	}
	return TMX_OK;
}

// GridPatch::GetDataTracers(instance) [nt][na][nb][L] <-> tracer slabs
extern "C" int tmx_upload_tracers(tmx_engine * e, int patch, int instance, const double * tracers) {
	int r = check_state_args(e, patch, instance);
	if (r) return r;
	REQUIRE(e->nt > 0 && tracers, TMX_ERR_INVALID, "tmx_upload_tracers: engine has no tracers / null array");
	const PatchInfo & P = e->patches[patch];
	const int L = e->L, na = P.na, nb = P.nb, nq = e->nt * L;
	const int ncp = P.nea * P.neb * TMX_NQ, c0 = P.elem_base * TMX_NQ;
	std::vector<double> buf((size_t)nq * ncp);
	for (int i = 1; i < na - 1; i++) for (int j = 1; j < nb - 1; j++) {
		const int c = col_of(P, i, j) - c0;
		for (int v = 0; v < e->nt; v++) for (int k = 0; k < L; k++)
			buf[(size_t)(v * L + k) * ncp + c] = tracers[(((size_t)v * na + i) * nb + j) * L + k];
	}
	HIPCHK(hipStreamSynchronize(e->stream));
	HIPCHK(hipMemcpy2D(e->d_state + (size_t)instance * e->inst_stride + (size_t)(5 * L + 1) * e->NS + c0, (size_t)e->NS * sizeof(double),
		buf.data(), (size_t)ncp * sizeof(double), (size_t)ncp * sizeof(double), nq, hipMemcpyHostToDevice));
	return TMX_OK;
}

extern "C" int tmx_download_tracers(tmx_engine * e, int patch, int instance, double * tracers) {
	int r = check_state_args(e, patch, instance, true);
	if (r) return r;
	REQUIRE(e->nt > 0 && tracers, TMX_ERR_INVALID, "tmx_download_tracers: engine has no tracers / null array");
	const PatchInfo & P = e->patches[patch];
	const int L = e->L, na = P.na, nb = P.nb, nq = e->nt * L;
	const int ncp = P.nea * P.neb * TMX_NQ, c0 = P.elem_base * TMX_NQ;
	std::vector<double> buf((size_t)nq * ncp);
	HIPCHK(hipStreamSynchronize(e->stream));
	HIPCHK(hipMemcpy2D(buf.data(), (size_t)ncp * sizeof(double), e->d_state + (size_t)instance * e->inst_stride + (size_t)(5 * L + 1) * e->NS + c0,
		(size_t)e->NS * sizeof(double), (size_t)ncp * sizeof(double), nq, hipMemcpyDeviceToHost));
	for (int i = 1; i < na - 1; i++) for (int j = 1; j < nb - 1; j++) {
		const int c = col_of(P, i, j) - c0;
		for (int v = 0; v < e->nt; v++) for (int k = 0; k < L; k++)
			tracers[(((size_t)v * na + i) * nb + j) * L + k] = buf[(size_t)(v * L + k) * ncp + c];
	}
	return TMX_OK;
}

extern "C" int tmx_download_state(tmx_engine * e, int patch, int instance, double * node, double * redge) {
	int r = check_state_args(e, patch, instance, true);
	if (r) return r;
	REQUIRE(node && (redge || e->sw), TMX_ERR_INVALID, "tmx_download_state: null array");
	const PatchInfo & P = e->patches[patch];
	const int L = e->L, na = P.na, nb = P.nb;
	const int ncp = P.nea * P.neb * TMX_NQ, c0 = P.elem_base * TMX_NQ;
	const int nstate = 5 * L + 1;
	double * bufp = stage_buffer(e, (size_t)nstate * ncp);
	REQUIRE(bufp, TMX_ERR_DEVICE, "cannot allocate the pinned staging buffer");
	struct { double * p; double * data() const { return p; } } buf = { bufp };
	HIPCHK(hipStreamSynchronize(e->stream));
	HIPCHK(hipMemcpy2D(buf.data(), (size_t)ncp * sizeof(double), e->d_state + (size_t)instance * e->inst_stride + c0,
		(size_t)e->NS * sizeof(double), (size_t)ncp * sizeof(double), nstate, hipMemcpyDeviceToHost));
	const int nodevar[4] = { 0, 1, 2, 4 };
	const double * ops = e->h_ops.data();
	auto opc = [&](int op, int k, int off) { return ops[((size_t)op * (L + 1) + k) * TMX_OPW + (off + 2)]; };
	const int * hoff = host_offsets(e, patch).data();
	const size_t nn = (size_t)na * nb;
	const bool sw = e->sw;
	if (!sw && e->track_surface) {
		// tracked surface slots back into the interface-level-0 entries of rho and rho*theta (see surface_copy)
		std::vector<double> ss((size_t)2 * ncp);
		HIPCHK(hipMemcpy2D(ss.data(), (size_t)ncp * sizeof(double), e->d_state + (size_t)instance * e->inst_stride + (size_t)e->nslab * e->NS + c0,
			(size_t)e->NS * sizeof(double), (size_t)ncp * sizeof(double), 2, hipMemcpyDeviceToHost));
		for (int c = 0; c < ncp; c++) {
			redge[((size_t)4 * nn + hoff[c]) * (L + 1)] = ss[c];
			redge[((size_t)2 * nn + hoff[c]) * (L + 1)] = ss[(size_t)ncp + c];
		}
	}
	host_parallel((ncp + 63) / 64, [&](int ta, int tb) {
		for (int t = ta; t < tb; t++) {
			const int ca = t * 64, cb = std::min(ncp, ca + 64);
			if (sw) {
				for (int v = 0; v < 3; v++) xpose_to_host(node, (size_t)v * nn, 1, buf.data(), v, ncp, hoff, ca, cb);
				continue;
			}
			for (int v = 0; v < 4; v++) xpose_to_host(node, (size_t)nodevar[v] * nn, L, buf.data(), v * L, ncp, hoff, ca, cb);
			xpose_to_host(redge, (size_t)3 * nn, L + 1, buf.data(), 4 * L, ncp, hoff, ca, cb);
			// derived slots the reference keeps beside the prognostic ones (HorizontalDynamicsFEM.cpp:817-831):
			// W on levels, U and V on interfaces, from the columns just written (contiguous on the host)
			for (int c = ca; c < cb; c++) {
				const size_t ho = hoff[c];
				const double * colU = node + ((size_t)0 * nn + ho) * L, * colV = node + ((size_t)1 * nn + ho) * L;
				const double * colW = redge + ((size_t)3 * nn + ho) * (L + 1);
				double * wn = node + ((size_t)3 * nn + ho) * L;
				double * ue_ = redge + ((size_t)0 * nn + ho) * (L + 1), * ve_ = redge + ((size_t)1 * nn + ho) * (L + 1);
				for (int k = 0; k < L; k++) {
					double w = 0.0;
					w += opc(TMX_OP_INTERP_REDGE_TO_NODE, k, 0) * colW[k];
					w += opc(TMX_OP_INTERP_REDGE_TO_NODE, k, 1) * colW[k + 1];
					wn[k] = w;
				}
				for (int k = 0; k <= L; k++) {
					double ue = 0.0, ve = 0.0;
					for (int off = -2; off <= 1; off++) {
						const int l = k + off;
						if (l < 0 || l >= L) continue;
						const double cc = opc(TMX_OP_INTERP_NODE_TO_REDGE, k, off);
						if (cc == 0.0) continue;
						ue += cc * colU[l]; ve += cc * colV[l];
					}
					ue_[k] = ue; ve_[k] = ve;
				}
			}
		}
	});
	return TMX_OK;
}

// ---------------------------------------------------------------------------------------------
// Restart image (second half): the bytes of GridPatch::GetDataContainerActiveState() (GridPatch.cpp:359-361,387),
// which is what OutputManagerComposite::Output writes per patch (OutputManagerComposite.cpp:331-349) and what a restart reads
// back.  The transposition from the slab layout runs on the device; the host sees ONE contiguous copy per patch.

static size_t active_state_doubles(const tmx_engine * e, const PatchInfo & P) {
	const size_t nn = (size_t)P.na * P.nb;
	return 5 * nn * e->L + 5 * nn * (e->L + 1) + (size_t)e->nt * nn * e->L;
}

extern "C" long long tmx_active_state_bytes(tmx_engine * e, int patch) {
	if (!e || patch < 0 || patch >= e->cfg.n_patches || e->sw) return -1;
	return (long long)(sizeof(double) * (1 + active_state_doubles(e, e->patches[patch])));      // 8-byte DataArray1D<int> chunk in front
}

static int image_buffer(tmx_engine * e, size_t n) {
	if (e->image_n < n) {
		if (e->d_image) { hipFree(e->d_image); e->hbm_bytes -= e->image_n * sizeof(double); }
		e->d_image = nullptr; e->image_n = 0;
		HIPCHK(hipMalloc((void **)&e->d_image, n * sizeof(double)));
		e->image_n = n; e->hbm_bytes += n * sizeof(double);
	}
	return TMX_OK;
}

extern "C" int tmx_pack_active_state(tmx_engine * e, int patch, int instance, void * dst, size_t dst_bytes) {
	int r = check_state_args(e, patch, instance, true);
	if (r) return r;
	REQUIRE(!e->sw, TMX_ERR_UNSUPPORTED, "restart image with the shallow-water equation set is not supported");
	const PatchInfo & P = e->patches[patch];
	const size_t nd = active_state_doubles(e, P);
	REQUIRE(dst && dst_bytes == sizeof(double) * (1 + nd), TMX_ERR_INVALID, "tmx_pack_active_state: %zu bytes given, the container of patch %d has %zu",
		dst_bytes, patch, sizeof(double) * (1 + nd));
	if ((r = image_buffer(e, nd))) return r;
	HIPCHK(hipMemsetAsync(e->d_image, 0, nd * sizeof(double), e->stream));       // halo ring and the entries nothing on the path reads
	tmxk_active_state_image(e, make_params(e), true, P.elem_base * TMX_NQ, P.nea * P.neb * TMX_NQ, P.na, P.nb, P.neb,
		e->d_state + (size_t)instance * e->inst_stride, e->track_surface ? e->d_state + (size_t)instance * e->inst_stride + (size_t)e->nslab * e->NS : nullptr, e->d_image);
	if ((r = launch_check("pack_active_state"))) return r;
	unsigned char * out = (unsigned char *)dst;
	HIPCHK(hipMemcpyAsync(out + sizeof(double), e->d_image, nd * sizeof(double), hipMemcpyDeviceToHost, e->stream));
	HIPCHK(hipStreamSynchronize(e->stream));
	memset(out, 0, sizeof(double));
	const int ix = patch; memcpy(out, &ix, sizeof(int));       // m_iActiveStatePatchIx (GridPatch.cpp:359)
	return TMX_OK;
}

extern "C" int tmx_unpack_active_state(tmx_engine * e, int patch, int instance, const void * src, size_t src_bytes) {
	int r = check_state_args(e, patch, instance);
	if (r) return r;
	REQUIRE(!e->sw, TMX_ERR_UNSUPPORTED, "restart image with the shallow-water equation set is not supported");
	const PatchInfo & P = e->patches[patch];
	const size_t nd = active_state_doubles(e, P);
	REQUIRE(src && src_bytes == sizeof(double) * (1 + nd), TMX_ERR_INVALID, "tmx_unpack_active_state: %zu bytes given, the container of patch %d has %zu",
		src_bytes, patch, sizeof(double) * (1 + nd));
	int ix = -1; memcpy(&ix, src, sizeof(int));
	REQUIRE(ix == patch, TMX_ERR_INVALID, "tmx_unpack_active_state: the image is of patch %d, not %d", ix, patch);
	if ((r = image_buffer(e, nd))) return r;
	HIPCHK(hipStreamSynchronize(e->stream));
	HIPCHK(hipMemcpyAsync(e->d_image, (const unsigned char *)src + sizeof(double), nd * sizeof(double), hipMemcpyHostToDevice, e->stream));
	tmxk_active_state_image(e, make_params(e), false, P.elem_base * TMX_NQ, P.nea * P.neb * TMX_NQ, P.na, P.nb, P.neb,
		e->d_state + (size_t)instance * e->inst_stride, e->d_state + (size_t)instance * e->inst_stride + (size_t)e->nslab * e->NS, e->d_image);
	if ((r = launch_check("unpack_active_state"))) return r;
	HIPCHK(hipStreamSynchronize(e->stream));      // the caller may reuse src
	return TMX_OK;
}

// ---------------------------------------------------------------------------------------------
// multi-GPU

extern "C" int tmx_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
	return n;
}

extern "C" int tmx_comm_unique_id(unsigned char id[128]) {
	int r = load_rccl();
	if (r) return r;
	nccl_uid u;
	NCCLCHK(g_nccl.GetUniqueId(&u));
	memcpy(id, u.internal, 128);
	return TMX_OK;
}

extern "C" int tmx_comm_init(tmx_engine * e, const unsigned char id[128]) {
	if (e && !e->xstream && e->cfg.device != -2 && !e->opt_no_exchange_overlap) {
		// second stream + events for the exchange / interior-DSS overlap
		if (hipStreamCreateWithFlags(&e->xstream, hipStreamNonBlocking) != hipSuccess) e->xstream = nullptr;
		else { hipEventCreateWithFlags(&e->ev_pack, hipEventDisableTiming); hipEventCreateWithFlags(&e->ev_recv, hipEventDisableTiming); }
	}
	REQUIRE(e && id && !plan_only(e), TMX_ERR_INVALID, "tmx_comm_init: bad argument");
	int r = load_rccl();
	if (r) return r;
	HIPCHK(hipSetDevice(e->device));
	nccl_uid u;
	memcpy(u.internal, id, 128);
	{
		const int nr = g_nccl.CommInitRank(&e->comm, e->cfg.n_ranks, u, e->cfg.rank);
		if (nr != 0) {
			// the usual cause: several ranks of one node on the same HIP device (RCCL: "Duplicate GPU detected")
			tmx_set_error("ncclCommInitRank failed (RCCL error %d) for rank %d of %d on HIP device %d: every rank needs a GPU of its own "
				"-- set tmx_config.device per rank (tmx_device_count(), node-local rank) or restrict HIP_VISIBLE_DEVICES per rank",
				nr, e->cfg.rank, e->cfg.n_ranks, e->device);
			e->comm = nullptr;
			return TMX_ERR_DEVICE;
		}
	}
	return TMX_OK;
}

// Peer-to-peer halo transport: instead of RCCL send/recv, every rank maps the ghost buffers of its neighbour ranks (HIP IPC)
// and its gather kernel writes the boundary columns straight into them; an arrival counter per (parity, source rank) in the
// same block orders the two sides.  Set-up: every rank exports a blob, the caller all-gathers the blobs (any transport: the
// reference's MPI, torch.distributed) and hands all of them to tmx_halo_p2p_connect; before tmx_destroy the caller lets every
// rank finish (a barrier), since neighbours write into this rank's block.  The reference's exchange this replaces:
// Connectivity.cpp:928-1120 (ExchangeBuffer pack / MPI_Isend / MPI_Irecv / unpack), Grid.cpp:627-685.
struct p2p_blob_head { hipIpcMemHandle_t handle; unsigned long long ghost_doubles; int n_ranks, rank; char pci[16]; };      // pci: bus id of the exporting device

extern "C" int tmx_halo_p2p_blob_bytes(tmx_engine * e) {
	if (!e || !e->finalized) return -1;
	return (int)(sizeof(p2p_blob_head) + sizeof(int) * (e->cfg.n_ranks + 1));
}

extern "C" int tmx_halo_p2p_export(tmx_engine * e, unsigned char * blob) {
	int r; if ((r = check_ready(e))) return r;
	REQUIRE(blob, TMX_ERR_INVALID, "tmx_halo_p2p_export: null blob");
	REQUIRE(!plan_only(e) && e->cfg.n_ranks > 1 && !e->lb, TMX_ERR_INVALID, "tmx_halo_p2p_export needs a device engine of a multi-rank layout");
	HIPCHK(hipSetDevice(e->device));
	const size_t gd = (size_t)e->nslab * e->nghost_pad;
	if (!e->p2p_block) {
		e->p2p_block_bytes = p2p_header_bytes(e->cfg.n_ranks) + 2 * gd * sizeof(double);
		// fine-grained: writes of other devices and the counters are visible without a cache flush on this side
		HIPCHK(hipExtMallocWithFlags(&e->p2p_block, e->p2p_block_bytes, hipDeviceMallocFinegrained));
		HIPCHK(hipMemset(e->p2p_block, 0, e->p2p_block_bytes));
		HIPCHK(hipDeviceSynchronize());
		e->hbm_bytes += e->p2p_block_bytes;
	}
	p2p_blob_head h;
	memset(&h, 0, sizeof(h));
	HIPCHK(hipIpcGetMemHandle(&h.handle, e->p2p_block));
	h.ghost_doubles = gd; h.n_ranks = e->cfg.n_ranks; h.rank = e->cfg.rank;
	if (hipDeviceGetPCIBusId(h.pci, (int)sizeof(h.pci), e->device) != hipSuccess) { (void)hipGetLastError(); h.pci[0] = 0; }
	h.pci[sizeof(h.pci) - 1] = 0;
	memcpy(blob, &h, sizeof(h));
	memcpy(blob + sizeof(h), e->recv_rank_off.data(), sizeof(int) * (e->cfg.n_ranks + 1));
	return TMX_OK;
}

extern "C" int tmx_halo_p2p_connect(tmx_engine * e, const unsigned char * blobs) {
	int r; if ((r = check_ready(e))) return r;
	REQUIRE(blobs && e->p2p_block, TMX_ERR_INVALID, "tmx_halo_p2p_connect: call tmx_halo_p2p_export first and pass the blobs of all ranks");
	REQUIRE(!e->p2p_connected, TMX_ERR_INVALID, "tmx_halo_p2p_connect: already connected");
	const int NR = e->cfg.n_ranks, me = e->cfg.rank;
	const size_t bb = (size_t)tmx_halo_p2p_blob_bytes(e), hb = p2p_header_bytes(NR);
	HIPCHK(hipSetDevice(e->device));
	e->p2p_peer.assign(NR, nullptr);
	std::vector<double *> dst(2 * (size_t)NR, nullptr);
	std::vector<unsigned long long *> flg(2 * (size_t)NR, nullptr);
	std::vector<int> peers;
	for (int rk = 0; rk < NR; rk++) {
		p2p_blob_head h;
		memcpy(&h, blobs + bb * rk, sizeof(h));
		const int * roff = (const int *)(blobs + bb * rk + sizeof(h));
		REQUIRE(h.n_ranks == NR && h.rank == rk, TMX_ERR_INVALID, "tmx_halo_p2p_connect: blob %d is from rank %d of %d", rk, h.rank, h.n_ranks);
		const int ns = e->send_rank_off[rk + 1] - e->send_rank_off[rk], nr = e->recv_rank_off[rk + 1] - e->recv_rank_off[rk];
		const int their = roff[me + 1] - roff[me];
		REQUIRE(rk == me || their == ns, TMX_ERR_INVALID, "rank %d sends %d columns to rank %d which expects %d", me, ns, rk, their);
		REQUIRE(rk == me || (ns > 0) == (nr > 0), TMX_ERR_INVALID, "halo between ranks %d and %d is one-sided (%d out, %d in)", me, rk, ns, nr);
		if (rk == me || ns == 0) continue;
		// a neighbour on another device of this node: the gather kernel will write into its memory, which needs peer access
		// (where this process can see that device at all; otherwise the mapping below is the test)
		if (h.pci[0]) {
			int their_dev = -1;
			if (hipDeviceGetByPCIBusId(&their_dev, h.pci) == hipSuccess && their_dev >= 0 && their_dev != e->device) {
				int can = 0;
				if (hipDeviceCanAccessPeer(&can, e->device, their_dev) != hipSuccess) { (void)hipGetLastError(); can = 0; }
				REQUIRE(can, TMX_ERR_COMM, "device %d (this rank) has no peer access to device %d (%s, rank %d): no peer-to-peer halo between them", e->device, their_dev, h.pci, rk);
			} else (void)hipGetLastError();
		}
		void * base = nullptr;
		const hipError_t oe = hipIpcOpenMemHandle(&base, h.handle, hipIpcMemLazyEnablePeerAccess);
		REQUIRE(oe == hipSuccess, TMX_ERR_COMM, "hipIpcOpenMemHandle of rank %d's halo block failed: %s (ranks of one process cannot map each other; "
			"HSA_ENABLE_IPC_MODE_LEGACY=0 is needed where the driver only supports dmabuf IPC)", rk, hipGetErrorString(oe));
		e->p2p_peer[rk] = base;
		peers.push_back(rk);
		for (int b = 0; b < 2; b++) {
			dst[(size_t)b * NR + rk] = (double *)((char *)base + hb) + (size_t)b * h.ghost_doubles + (size_t)e->nslab * roff[me];
			flg[(size_t)b * NR + rk] = (unsigned long long *)base + (size_t)b * NR + me;
		}
	}
	std::vector<int> sp(e->nsend), sw(e->nsend);
	for (int rk = 0; rk < NR; rk++)
		for (int t = e->send_rank_off[rk]; t < e->send_rank_off[rk + 1]; t++) { sp[t] = rk; sw[t] = t - e->send_rank_off[rk]; }
	size_t bytes = 0;
	if ((r = dev_upload(&e->d_p2p_dst, dst, &bytes)) || (r = dev_upload(&e->d_p2p_flag, flg, &bytes)) || (r = dev_upload(&e->d_send_peer, sp, &bytes))
		|| (r = dev_upload(&e->d_send_within, sw, &bytes)) || (r = dev_upload(&e->d_p2p_peers, peers, &bytes))) return r;
	e->hbm_bytes += bytes;
	e->p2p_npeers = (int)peers.size();
	if (!e->xstream && !e->opt_no_exchange_overlap) {
		if (hipStreamCreateWithFlags(&e->xstream, hipStreamNonBlocking) != hipSuccess) e->xstream = nullptr;
		else { hipEventCreateWithFlags(&e->ev_pack, hipEventDisableTiming); hipEventCreateWithFlags(&e->ev_recv, hipEventDisableTiming); }
	}
	e->d_ghost_own = e->d_ghost;
	e->p2p = true;
	e->p2p_connected = true;
	return TMX_OK;
}

// Switch between the two transports of a connected engine (both set up: tmx_comm_init and tmx_halo_p2p_connect), e.g. to time
// them against each other at start-up.  Every rank must switch at the same point of the program, with no exchange in flight.
extern "C" int tmx_halo_p2p_enable(tmx_engine * e, int on) {
	int r; if ((r = check_ready(e))) return r;
	REQUIRE(e->p2p_connected, TMX_ERR_INVALID, "tmx_halo_p2p_enable: tmx_halo_p2p_connect first");
	REQUIRE(on || e->comm, TMX_ERR_INVALID, "tmx_halo_p2p_enable(0): no RCCL communicator to fall back to (tmx_comm_init)");
	HIPCHK(hipStreamSynchronize(e->stream));
	if (e->xstream) HIPCHK(hipStreamSynchronize(e->xstream));
	e->p2p = on != 0;
	if (!e->p2p) e->d_ghost = e->d_ghost_own;
	return TMX_OK;
}

// After a failed exchange (tmx_sync returned TMX_ERR_COMM) the ranks' exchange counters disagree.  Once EVERY rank has
// returned from tmx_sync and the caller has put a barrier behind that (nobody is inside an exchange, nobody writes into a
// neighbour's block), each rank calls this: its arrival counters and its own exchange count start from zero again.  A second
// barrier, then the ranks may go on -- with either transport -- from a state they upload again.
extern "C" int tmx_halo_p2p_reset(tmx_engine * e) {
	int r; if ((r = check_ready(e))) return r;
	REQUIRE(e->p2p_connected, TMX_ERR_INVALID, "tmx_halo_p2p_reset: tmx_halo_p2p_connect first");
	HIPCHK(hipStreamSynchronize(e->stream));
	if (e->xstream) HIPCHK(hipStreamSynchronize(e->xstream));
	HIPCHK(hipMemset(e->p2p_block, 0, p2p_header_bytes(e->cfg.n_ranks)));
	HIPCHK(hipMemset(e->d_flag, 0, sizeof(int)));
	HIPCHK(hipDeviceSynchronize());
	e->p2p_seq = 0;
	return TMX_OK;
}

// ---------------------------------------------------------------------------------------------
// introspection

extern "C" long long tmx_info(tmx_engine * e, int what) {
	if (!e) return -1;
	switch (what) {
		case TMX_INFO_LOCAL_COLUMNS: return e->ncol;
		case TMX_INFO_UNIQUE_COLUMNS: return e->nunique;
		case TMX_INFO_DSS_GROUPS: return e->ngroups;
		case TMX_INFO_LOCAL_ELEMENTS: return e->ne_local;
		case TMX_INFO_GHOST_COLUMNS: return e->nghost;
		case TMX_INFO_HBM_BYTES: return (long long)e->hbm_bytes;
		case TMX_INFO_METRIC_CLOSED_FORM: return e->metric_closed ? 1 : 0;
		case TMX_INFO_EARLY_TILES: return e->split_stage ? e->n_quads_early : 0;
		case TMX_INFO_LATE_TILES: return e->split_stage ? e->n_quads_late : 0;
		case TMX_INFO_UNIQUE_LAYOUT: return e->u.built ? 1 : 0;
		case TMX_INFO_UNIQUE_INSTANCES: return e->u.n_uform;
		case TMX_INFO_UNIQUE_CONVERSIONS: return e->u.conversions;
		case TMX_INFO_PARTIAL_SLOTS: return e->u.built ? e->u.nslots : 0;
		case TMX_INFO_UNIQUE_DSS_GROUPS: return e->u.built ? e->u.ngroups : 0;
		case TMX_INFO_PREFIX_STAGES: return e->u.prefix_stages;
		case TMX_INFO_EXPERIMENTS_BUILD: return TMX_EXP;
		case TMX_INFO_MIXED_STEPS: return e->u.mixed_steps;
		case TMX_INFO_COLUMN_KERNEL: return e->vi_kernel_launched;
		case TMX_INFO_COLUMN_VARIANT: return e->vi_variant_launched;
		case TMX_INFO_STAGE_KERNEL: return e->stage_kernel_launched;
		case TMX_INFO_HYPERVIS_KERNEL: return e->hypervis_kernel_launched;
		case TMX_INFO_PHYSICS_KERNEL: return e->physics_kernel_launched;
		case TMX_INFO_TRACER_COLUMN_KERNEL: return e->vt_kernel_launched;
		case TMX_INFO_VERTICAL_KERNELS: {      // 12 bits per kernel, 0xfff: that one not launched yet
			const int * v = e->vwalk_launched;
			if (v[0] < 0 && v[1] < 0 && v[2] < 0) return -1;
			return (long long)(v[0] & 0xfff) | (long long)(v[1] & 0xfff) << 12 | (long long)(v[2] & 0xfff) << 24;
		}
		case TMX_INFO_COMM_RANKS: {      // what RCCL itself reports for the communicator (0: no communicator)
			int n = 0;
			if (e->comm && g_nccl.CommCount && g_nccl.CommCount(e->comm, &n) == 0) return n;
			return 0;
		}
		case TMX_INFO_SEND_COLUMNS: return e->nsend;
		case TMX_INFO_HALO_TRANSPORT: return (e->cfg.n_ranks == 1) ? 0 : (e->lb ? 3 : (e->p2p ? 2 : (e->comm ? 1 : 0)));
	}
	return -1;
}

// Diagnostic builds (-DTMX_H_TIMING): shader cycles per wavefront of the fused explicit kernel by phase, [16][8] (tmx_k_horizontal.hip)
extern "C" int tmx_debug_h_timing(tmx_engine * e, unsigned long long * out) {
	int r; if ((r = check_ready(e))) return r;
	HIPCHK(hipStreamSynchronize(e->stream));
	tmxk_h_timing_read(out);
	return TMX_OK;
}
// the same for the column-segment walk (tmx_k_hwalk.hip), [8][8]; padded to [16][8] like the above
extern "C" int tmx_debug_h_walk_timing(tmx_engine * e, unsigned long long * out) {
	int r; if ((r = check_ready(e))) return r;
	HIPCHK(hipStreamSynchronize(e->stream));
	tmxk_h_walk_timing_read(out);
	return TMX_OK;
}

// Host logic of the column walks, no device: the number of segments their launchers choose (walk_segments, tmx_internal.h)
extern "C" int tmx_debug_walk_segments(int option, int ntiles, int rows, int target_wavefronts) {
	return walk_segments(option, ntiles, rows, target_wavefronts);
}

// Would the launchers an ABI call is about to use fit?  Asked before the call's first kernel, so that a refused call leaves every instance as
// it was.  (Needs no device: the shape functions of tmx_internal.h on the engine's own numbers.)
int tmx_vertical_fit(tmx_engine * e, unsigned what) {
	if (e->sw) return TMX_OK;
	if ((what & TMX_FIT_VI) && e->nunique > 0) {
		const ViShape s = vi_shape(e->L, vi_shape_in(e, e->metric_closed));
		REQUIRE(s.fits(), TMX_ERR_UNSUPPORTED, "column solve (k_vi_pair): %d levels do not fit the LDS of a CU; this configuration serves up to %d levels", e->L, s.max_L);
	}
	if ((what & TMX_FIT_VT) && e->nt > 0 && e->nunique > 0) {
		const VtShape s = vt_solve_shape(e, false);
		REQUIRE(s.fits(), TMX_ERR_UNSUPPORTED, "tracer column update (k_vi_tracers_rows): %d levels do not fit the LDS of a CU; this configuration serves up to %d levels", e->L, s.max_L);
	}
	if ((what & TMX_FIT_VT_ALL) && e->nt > 0 && e->ncol > 0) {
		const VtShape s = vt_solve_shape(e, true);
		REQUIRE(s.fits(), TMX_ERR_UNSUPPORTED, "tracer column update (k_vi_tracers_rows): %d levels do not fit the LDS of a CU; this configuration serves up to %d levels", e->L, s.max_L);
	}
	if ((what & TMX_FIT_VT_EXPLICIT) && e->nt > 0 && e->ncol > 0 && e->opt_vt_column) {
		const VtColumnShape s = vt_column_shape(e->L);
		REQUIRE(s.fits(), TMX_ERR_UNSUPPORTED, "tracer column update (k_v_tracers_explicit_column, option vt_column): %d levels do not fit the LDS of a CU; this configuration serves up to %d levels",
			e->L, s.max_L);
	}
	return TMX_OK;
}
// what a whole step may launch (tmx_step): implicit mode the column solve and both forms of the tracer update, fully explicit mode the tracer kernel
unsigned tmx_vertical_fit_of_step(const tmx_engine * e) { return e->fully_explicit ? TMX_FIT_VT_EXPLICIT : (TMX_FIT_VI | TMX_FIT_VT | TMX_FIT_VT_ALL); }

// Host logic of the vertical launchers, no device (tmx_internal.h: vi_shape, vt_solve_shape, vwalk_shape, vt_column_shape)
extern "C" int tmx_debug_vertical_shape(tmx_engine * e, int launcher, int levels, const int * args, int nargs, long long out[4]) {
	REQUIRE(out && (e || levels >= 1) && (nargs == 0 || args), TMX_ERR_INVALID, "tmx_debug_vertical_shape: bad argument");
	auto arg = [&](int i, int dflt) { return i < nargs ? args[i] : dflt; };
	out[0] = out[1] = out[2] = out[3] = 0;
	if (e) {
		REQUIRE(e->finalized && launcher >= 0 && launcher <= 5, TMX_ERR_INVALID, "tmx_debug_vertical_shape: engine not finalized or unknown launcher %d", launcher);
		static const unsigned bit[6] = { TMX_FIT_VI, TMX_FIT_VT, 0, 0, 0, TMX_FIT_VT_EXPLICIT };
		const unsigned what = (launcher == 1 && arg(0, 0)) ? TMX_FIT_VT_ALL : bit[launcher];
		const int r = tmx_vertical_fit(e, what);
		levels = e->L;
		if (r) {      // the message is set; out[3]: the limit it names
			out[0] = -1;
			out[3] = launcher == 0 ? vi_shape(levels, vi_shape_in(e, e->metric_closed)).max_L : (launcher == 1 ? vt_solve_shape(e, arg(0, 0) != 0).max_L : vt_column_shape(levels).max_L);
			return r;
		}
	}
	switch (launcher) {
		case 0: {      // column solve: args = unique columns, columns per wavefront, closed-form metric, stream columns, vi_group, vi_group_max, vi_pair_workgroup, vi_producers, vi_ring_depth
			const ViShapeIn in = e ? vi_shape_in(e, e->metric_closed)
				: ViShapeIn{ arg(0, 0), arg(1, 64), arg(2, 1), arg(3, 1 << 30), arg(4, -1), arg(5, 6400), arg(6, 0), arg(7, 0), arg(8, 0), 1, 0 };
			REQUIRE(in.nunique >= 1 && in.cpw >= 1 && in.cpw <= 64, TMX_ERR_INVALID, "tmx_debug_vertical_shape: bad column-solve arguments");
			const ViShape s = vi_shape(levels, in);
			out[0] = s.kernel; out[1] = s.fits() ? (s.kernel == 1 ? (s.pairs | s.producers << 4 | s.ring << 8) : 0) : 0; out[2] = (long long)s.bytes; out[3] = s.max_L;
			return s.fits() ? 0 : 1;
		}
		case 1: {      // tracer column update: args = all columns, vt_rows, vt_row_lanes, vt_lw8, vt_lanes
			const bool all = arg(0, 0) != 0;
			const VtShape s = e ? vt_solve_shape(e, all) : vt_solve_shape(levels, arg(1, 1), arg(2, 0), arg(3, -1), all ? 64 : arg(4, 16));
			out[0] = s.nr; out[1] = s.lwb; out[2] = (long long)s.bytes; out[3] = s.max_L;
			return s.fits() ? 0 : 1;
		}
		case 2: case 3: case 4: {      // the walks of V.StepExplicit (U,V), of the explicit tracer update, of the explicitly evaluated implicit terms: args = option, tiles, with U,V
			const int which = launcher - 2;
			const int opt = e ? (which == TMX_WALK_VX ? e->opt_vx_walk : (which == TMX_WALK_VT ? e->opt_vt_walk : e->opt_vite_walk)) : arg(0, -1000);
			const WalkShape s = vwalk_shape(which, levels, opt, e ? (e->ncol + 63) / 64 : arg(1, 1), arg(2, 0) != 0);
			out[0] = s.nseg; out[2] = (long long)s.bytes;
			return 0;
		}
		case 5: {      // option "vt_column"
			const VtColumnShape s = vt_column_shape(levels);
			out[0] = s.lw; out[2] = (long long)s.bytes; out[3] = s.max_L;
			return s.fits() ? 0 : 1;
		}
	}
	REQUIRE(false, TMX_ERR_INVALID, "tmx_debug_vertical_shape: unknown launcher %d", launcher);
}

// Statistics of the two-wavefront column kernel: how many pivot steps found the same pivot row in all 64 columns of a
// wavefront (the renaming path) out of all pivot steps.  enable = 1 starts counting (zeroed), 0 stops; out (may be NULL)
// receives {uniform, total} accumulated so far.
extern "C" int tmx_debug_pivot_stats(tmx_engine * e, int enable, unsigned long long out[2]) {
	int r; if ((r = check_ready(e))) return r;
	HIPCHK(hipStreamSynchronize(e->stream));
	if (out) {
		out[0] = out[1] = 0;
		if (e->d_pivot_stats) HIPCHK(hipMemcpy(out, e->d_pivot_stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	}
#ifdef TMX_PAIR_TIMING
	// diagnostic builds (tools/vi_timing.py): the column kernel leaves one record of cycle counts per wavefront behind the two counters
	const size_t stat_words = 2 + 8 * 4096;
	if (e->d_pivot_stats && !enable) {
		std::vector<unsigned long long> rec(stat_words);
		HIPCHK(hipMemcpy(rec.data(), e->d_pivot_stats, stat_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
		for (size_t w = 0; w < 4096; w++) {
			const unsigned long long * q = &rec[2 + 8 * w];
			if (q[0]) fprintf(stderr, "pairtiming wave %zu role %llu hw_id %llx xcc %llu work %llu wait %llu forward %llu back %llu\n", w, q[0] - 1, q[1], q[2], q[3], q[4], q[5], q[6]);
		}
		if (e->vi_split_back) {      // fill-in masks of three column groups (which U-row entries exist), one line per group
			const int n = TMX_FTOT * (e->L + 1);
			for (int g : { 0, 100, 400 }) {
				std::vector<int> m(n);
				HIPCHK(hipMemcpy(m.data(), (const int *)e->d_rhs + (size_t)g * n, n * sizeof(int), hipMemcpyDeviceToHost));
				fprintf(stderr, "umask group %d:", g);
				for (int j = 0; j < n; j++) fprintf(stderr, " %x", m[j] >> 4);
				fprintf(stderr, "\n");
			}
		}
	}
#else
	const size_t stat_words = 2;
#endif
	if (enable && !e->d_pivot_stats) { HIPCHK(hipMalloc((void **)&e->d_pivot_stats, stat_words * sizeof(unsigned long long))); HIPCHK(hipMemset(e->d_pivot_stats, 0, stat_words * sizeof(unsigned long long))); }
	if (!enable && e->d_pivot_stats) { (void)hipFree(e->d_pivot_stats); e->d_pivot_stats = nullptr; }
	return TMX_OK;
}

extern "C" int tmx_profile_enable(tmx_engine * e, int on) {
	REQUIRE(e, TMX_ERR_INVALID, "null engine");
	e->prof = (on != 0);
	return TMX_OK;
}

extern "C" int tmx_profile_get(tmx_engine * e, int kernel, double * total_ms, long long * launches) {
	REQUIRE(e && kernel >= 0 && kernel < TMX_K_COUNT, TMX_ERR_INVALID, "bad kernel id");
	if (!plan_only(e) && e->stream) { hipStreamSynchronize(e->stream); prof_collect(e); }
	if (total_ms) *total_ms = e->prof_slots[kernel].ms;
	if (launches) *launches = e->prof_slots[kernel].n;
	return TMX_OK;
}

extern "C" int tmx_profile_reset(tmx_engine * e) {
	REQUIRE(e, TMX_ERR_INVALID, "null engine");
	if (!plan_only(e) && e->stream) { hipStreamSynchronize(e->stream); prof_collect(e); }
	for (int i = 0; i < TMX_K_COUNT; i++) e->prof_slots[i] = ProfSlot();
	return TMX_OK;
}

