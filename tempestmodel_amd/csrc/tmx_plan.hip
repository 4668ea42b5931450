// tmx_plan.hip -- tmx_finalize: the element-major plan of a rank (DSS groups in the reference's averaging order, exchange lists, unique
// columns of the implicit solve, launch tables), built on the host (build_plan: plan-only engines too), then the device buffers
// (upload_plan: device engines only); and the introspection of the plan (tmx_plan_get, tmx_plan_get_matrices, tmx_debug_unique_tables).
// The node-unique layout has the same shape in tmx_unique.hip: tmxu_tables, tmxu_build.
#include "tmx_hostshared.h"

// ---------------------------------------------------------------------------------------------
// the plan, host only

struct NodeRef { int patch, i, j; };

// every node of every patch (halo ring included), numbered patch by patch, row-major in (i, j)
struct Nodes {
	const tmx_engine * e;
	std::vector<size_t> poff;
	explicit Nodes(const tmx_engine * e_) : e(e_), poff(e_->cfg.n_patches + 1, 0) {
		for (int p = 0; p < e->cfg.n_patches; p++) poff[p + 1] = poff[p] + (size_t)e->patches[p].na * e->patches[p].nb;
	}
	int id(int p, int i, int j) const { return (int)(poff[p] + (size_t)i * e->patches[p].nb + j); }
	NodeRef ref(int id) const {
		const int p = (int)(std::upper_bound(poff.begin(), poff.end(), (size_t)id) - poff.begin()) - 1;
		const int loc = id - (int)poff[p];
		return NodeRef{ p, loc / e->patches[p].nb, loc % e->patches[p].nb };
	}
	bool local(int id) const { return e->patches[ref(id).patch].owner == e->cfg.rank; }
	int col(int id) const { const NodeRef nr = ref(id); return col_of(e->patches[nr.patch], nr.i, nr.j); }      // of a local node
};
typedef std::vector<std::vector<int>> Groups;      // the node ids of every DSS group that has a member on this rank

static int uf_find(std::vector<int> & par, int x) {
	while (par[x] != x) { par[x] = par[par[x]]; x = par[x]; }
	return x;
}

// DSS groups (union-find over the element seams and the halo rings), their order, and the exchange lists.
// ghost_index: node id of a remote copy -> its place in the ghost buffer
static int build_groups(tmx_engine * e, const Nodes & N, Groups & groups, std::map<int, int> & ghost_index) {
	const int np = e->cfg.n_patches, me = e->cfg.rank, NR = e->cfg.n_ranks;
	PlanHost & plan = e->plan;
	// ---- union-find over all interior nodes of all patches
	std::vector<int> par(N.poff[np]);
	std::iota(par.begin(), par.end(), 0);
	auto unite = [&](int a, int b) { a = uf_find(par, a); b = uf_find(par, b); if (a != b) par[std::max(a, b)] = std::min(a, b); };
	for (int p = 0; p < np; p++) {
		const PatchInfo & P = e->patches[p];
		for (int a = 1; a < P.nea; a++) for (int j = 1; j < P.nb - 1; j++) unite(N.id(p, a * TMX_NP, j), N.id(p, a * TMX_NP + 1, j));
		for (int b = 1; b < P.neb; b++) for (int i = 1; i < P.na - 1; i++) unite(N.id(p, i, b * TMX_NP), N.id(p, i, b * TMX_NP + 1));
		for (size_t m = 0; m < P.hi.size(); m++) {
			if (P.hsp[m] < 0) continue;
			const int xi = std::min(std::max(P.hi[m], 1), P.na - 2), xj = std::min(std::max(P.hj[m], 1), P.nb - 2);
			const PatchInfo & Q = e->patches[P.hsp[m]];
			REQUIRE(P.hsi[m] >= 1 && P.hsi[m] < Q.na - 1 && P.hsj[m] >= 1 && P.hsj[m] < Q.nb - 1, TMX_ERR_INVALID, "halo source is not an interior node");
			unite(N.id(p, xi, xj), N.id(P.hsp[m], P.hsi[m], P.hsj[m]));
		}
	}
	// members per root
	std::map<int, std::vector<int>> comps;
	for (int p = 0; p < np; p++) {
		const PatchInfo & P = e->patches[p];
		for (int i = 1; i < P.na - 1; i++) for (int j = 1; j < P.nb - 1; j++) {
			const bool edge = ((i - 1) % TMX_NP == 0) || ((i - 1) % TMX_NP == TMX_NP - 1) || ((j - 1) % TMX_NP == 0) || ((j - 1) % TMX_NP == TMX_NP - 1);
			if (!edge) continue;
			comps[uf_find(par, N.id(p, i, j))].push_back(N.id(p, i, j));
		}
	}
	// ---- exchange lists: (owner s -> needer r) node ids
	std::vector<std::vector<int>> send_to(NR), recv_from(NR);
	for (auto & kv : comps) {
		std::vector<int> & ids = kv.second;
		if (ids.size() < 2) continue;
		REQUIRE(ids.size() <= 4, TMX_ERR_INVALID, "DSS group with %d members (connectivity is inconsistent)", (int)ids.size());
		std::sort(ids.begin(), ids.end());
		bool local = false;
		for (int id : ids) if (N.local(id)) local = true;
		if (!local) continue;
		groups.push_back(ids);
		for (int a : ids) for (int b : ids) {
			const int oa = e->patches[N.ref(a).patch].owner, ob = e->patches[N.ref(b).patch].owner;
			if (oa == me && ob != me) send_to[ob].push_back(a);
			if (oa != me && ob == me) recv_from[oa].push_back(a);
		}
	}
	// order the groups by the device column of their first local member: consecutive lanes of the
	// DSS kernel then touch the same 128-byte element rows (element-major locality)
	{
		std::vector<std::pair<int, int>> key(groups.size());
		for (size_t g = 0; g < groups.size(); g++) {
			int best = 0x7fffffff;
			for (int id : groups[g]) if (N.local(id)) best = std::min(best, N.col(id));
			key[g] = { best, (int)g };
		}
		// groups with a member on another rank go last: the DSS of the others does not wait for the exchange; groups whose
		// copies all lie in ONE patch go first: the fused hyperviscosity kernel averages those itself (k_hypervis_block)
		std::vector<char> remote(groups.size(), 0);      // 0: one patch, 1: several patches of this rank, 2: a member on another rank
		for (size_t g = 0; g < groups.size(); g++) {
			const int p0 = N.ref(groups[g][0]).patch;
			for (int id : groups[g]) {
				if (!N.local(id)) remote[g] = 2;
				// (the in-patch class only with the fused hyperviscosity kernel: taking the patch-edge groups out of the column
				// order costs k_dss 10 % -- 0.45 instead of 0.41 ms per step at ne30 -- when it still averages all of them)
				else if (e->hvis_block && N.ref(id).patch != p0 && remote[g] < 1) remote[g] = 1;
			}
		}
		std::sort(key.begin(), key.end(), [&](const std::pair<int, int> & a, const std::pair<int, int> & b) {
			if (remote[a.second] != remote[b.second]) return remote[a.second] < remote[b.second];
			return a < b;
		});
		Groups sorted(groups.size());
		e->ngroups_local = 0; e->ngroups_inpatch = 0;
		for (size_t g = 0; g < groups.size(); g++) {
			sorted[g] = groups[key[g].second];
			if (remote[key[g].second] < 2) e->ngroups_local++;
			if (e->hvis_block && remote[key[g].second] == 0) e->ngroups_inpatch++;
		}
		groups.swap(sorted);
	}
	e->send_rank_off.assign(NR + 1, 0); e->recv_rank_off.assign(NR + 1, 0);
	for (int rk = 0; rk < NR; rk++) {
		auto uniq = [](std::vector<int> & v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); };
		uniq(send_to[rk]); uniq(recv_from[rk]);
		e->send_rank_off[rk + 1] = e->send_rank_off[rk] + (int)send_to[rk].size();
		e->recv_rank_off[rk + 1] = e->recv_rank_off[rk] + (int)recv_from[rk].size();
		for (size_t t = 0; t < recv_from[rk].size(); t++) {
			ghost_index[recv_from[rk][t]] = e->recv_rank_off[rk] + (int)t;
			NodeRef nr = N.ref(recv_from[rk][t]);
			plan.recv_nodes.insert(plan.recv_nodes.end(), { nr.patch, nr.i, nr.j });
		}
		for (int id : send_to[rk]) {
			NodeRef nr = N.ref(id);
			plan.send_nodes.insert(plan.send_nodes.end(), { nr.patch, nr.i, nr.j });
			plan.send_cols.push_back(N.col(id));
		}
	}
	e->nsend = e->send_rank_off[NR];
	e->nghost = e->recv_rank_off[NR];
	e->nghost_pad = std::max(e->nghost, 1);
	return TMX_OK;
}

// Device group tables, in the reference's own averaging order.
// GridCSGLL::ApplyDSS (GridCSGLL.cpp:560-781) averages inside every patch (halo ring included) first across the
// alpha seams, then across the beta seams: a node shared by four copies becomes
//     0.5 * (0.5 * (x + x_alpha) + 0.5 * (x_beta + x_diag)),
// with the partners named in the frame of the node's OWN patch, halo values first rotated into that frame
// (TransformHaloVelocities, GridPatchCSGLL.cpp:1783-1924).  The sums commute but do not associate, so the copies
// of a node on patches whose alpha axes are not parallel (panel edges towards panels 4 / 5) receive results that
// differ in the last bit -- in the reference, and therefore here.  Per group the members are stored as
// [m0, alpha partner, beta partner, diagonal] of member m0, and every member gets a 2-bit pairing type relative to
// that order (0: {01|23}, 1: {02|13}, 2: {03|12}); cube corners (three copies, (1/3) * ((x + x_alpha) + x_beta),
// :735-781) get the order of their two partners (0: next, previous; 1: previous, next).  The covector matrices are
// kept per (member, partner): exactly the matrix of the ring entry through which the member's patch sees the partner.
static int build_group_tables(tmx_engine * e, const Nodes & N, const Groups & groups, const std::map<int, int> & ghost_index) {
	const int np = e->cfg.n_patches;
	PlanHost & plan = e->plan;
	std::vector<std::vector<int>> ring(np);
	for (int p = 0; p < np; p++) {
		const PatchInfo & P = e->patches[p];
		ring[p].assign((size_t)P.na * P.nb, -1);
		for (size_t h = 0; h < P.hi.size(); h++) ring[p][(size_t)P.hi[h] * P.nb + P.hj[h]] = (int)h;
	}
	// node id seen by patch p at extended (ring included) position (i, j); h = ring entry or -1
	auto ext = [&](int p, int i, int j, int & h) -> int {
		const PatchInfo & P = e->patches[p];
		h = -1;
		if (i >= 1 && i < P.na - 1 && j >= 1 && j < P.nb - 1) return N.id(p, i, j);
		h = ring[p][(size_t)i * P.nb + j];
		if (h < 0 || P.hsp[h] < 0) { h = -1; return -1; }
		return N.id(P.hsp[h], P.hsi[h], P.hsj[h]);
	};
	auto seam = [&](int c) -> int { const int q = (c - 1) % TMX_NP; return (q == 0) ? c - 1 : ((q == TMX_NP - 1) ? c + 1 : -1); };
	struct Roles { int id[3]; int h[3]; };      // alpha partner, beta partner, diagonal: node id (-1 none) and ring entry
	auto roles_of = [&](int id) -> Roles {
		const NodeRef nr = N.ref(id);
		Roles r;
		const int ia = seam(nr.i), jb = seam(nr.j);
		r.id[0] = (ia >= 0) ? ext(nr.patch, ia, nr.j, r.h[0]) : (r.h[0] = -1, -1);
		r.id[1] = (jb >= 0) ? ext(nr.patch, nr.i, jb, r.h[1]) : (r.h[1] = -1, -1);
		r.id[2] = (ia >= 0 && jb >= 0) ? ext(nr.patch, ia, jb, r.h[2]) : (r.h[2] = -1, -1);
		return r;
	};
	e->ngroups = (int)groups.size();
	plan.grp_cols.assign((size_t)e->ngroups * 4, -1);
	plan.grp_n.assign(e->ngroups, 0);
	plan.grp_x.assign(e->ngroups, -1);
	plan.grp_type.assign(e->ngroups, 0);
	for (int g = 0; g < e->ngroups; g++) {
		std::vector<int> ids = groups[g];
		const int n = (int)ids.size();
		// order: [m0, alpha partner, beta partner, diagonal] of the first member
		{
			const Roles r0 = roles_of(ids[0]);
			std::vector<int> ord(1, ids[0]);
			if (n == 4) { ord.push_back(r0.id[0]); ord.push_back(r0.id[1]); ord.push_back(r0.id[2]); }
			else if (n == 3) { ord.push_back(r0.id[0]); ord.push_back(r0.id[1]); }
			else ord.push_back((r0.id[0] >= 0) ? r0.id[0] : r0.id[1]);
			std::vector<int> chk = ord; std::sort(chk.begin(), chk.end());
			REQUIRE(chk == ids, TMX_ERR_INVALID, "DSS group %d: the seam / halo partners of a node are not the group's members", g);
			ids = ord;
		}
		plan.grp_n[g] = n;
		auto pos = [&](int id) { for (int t = 0; t < n; t++) if (ids[t] == id) return t; return -1; };
		double M[64];
		for (int t = 0; t < 16; t++) { M[4 * t] = 1; M[4 * t + 1] = 0; M[4 * t + 2] = 0; M[4 * t + 3] = 1; }
		bool cross = false;
		int type = 0;
		for (int m = 0; m < n; m++) {
			const NodeRef nr = N.ref(ids[m]);
			const PatchInfo & P = e->patches[nr.patch];
			plan.grp_cols[(size_t)g * 4 + m] = N.local(ids[m]) ? N.col(ids[m]) : e->NS + ghost_index.at(ids[m]);
			const Roles r = roles_of(ids[m]);
			int ty = 0;
			if (n == 4) {
				const int pa = pos(r.id[0]), pb = pos(r.id[1]), pd = pos(r.id[2]);
				REQUIRE(pa >= 0 && pb >= 0 && pd >= 0 && pa != pb && pa != pd && pb != pd && pa != m && pb != m && pd != m,
					TMX_ERR_INVALID, "DSS group %d: inconsistent partners of member %d", g, m);
				const int lo = std::min(m, pa), hi = std::max(m, pa);
				ty = ((lo == 0 && hi == 1) || (lo == 2 && hi == 3)) ? 0 : (((lo == 0 && hi == 2) || (lo == 1 && hi == 3)) ? 1 : 2);
			} else if (n == 3) {
				const int pa = pos(r.id[0]), pb = pos(r.id[1]);
				REQUIRE(pa >= 0 && pb >= 0 && pa != pb && pa != m && pb != m && r.id[2] < 0, TMX_ERR_INVALID, "DSS group %d: inconsistent cube-corner partners", g);
				ty = (pa == (m + 1) % 3) ? 0 : 1;
			} else {
				const int pp = pos((r.id[0] >= 0) ? r.id[0] : r.id[1]);
				REQUIRE(pp == 1 - m && (r.id[0] < 0 || r.id[1] < 0), TMX_ERR_INVALID, "DSS group %d: inconsistent edge partners", g);
			}
			type |= ty << (2 * m);
			// covector matrices: partner seen through a ring entry whose source lies on another panel
			for (int t = 0; t < 3; t++) {
				if (r.id[t] < 0 || r.h[t] < 0) continue;
				if (P.hspanel[r.h[t]] == P.panel) continue;
				REQUIRE(!P.htrans.empty(), TMX_ERR_INVALID, "covector transforms of patch %d not set", nr.patch);
				memcpy(M + (m * 4 + pos(r.id[t])) * 4, &P.htrans[4 * (size_t)r.h[t]], 4 * sizeof(double));
				cross = true;
			}
		}
		plan.grp_type[g] = type;
		if (cross) {
			plan.grp_x[g] = (int)(plan.xmat.size() / 64);
			plan.xmat.insert(plan.xmat.end(), M, M + 64);
		}
	}
	e->nxgroups = (int)(plan.xmat.size() / 64);
	return TMX_OK;
}

// unique columns of the implicit solve and their in-patch duplicates (VerticalDynamicsFEM.cpp:1315-1337, 1543-1633)
static void build_unique_columns(tmx_engine * e) {
	PlanHost & plan = e->plan;
	for (int p : e->local_patches) {
		const PatchInfo & P = e->patches[p];
		for (int a = 0; a < P.nea; a++) for (int b = 0; b < P.neb; b++)
		for (int ii = 0; ii < TMX_NP; ii++) for (int jj = 0; jj < TMX_NP; jj++) {
			const bool ua = (ii < TMX_NP - 1) || (a == P.nea - 1), ub = (jj < TMX_NP - 1) || (b == P.neb - 1);
			if (!ua || !ub) continue;
			const int i = 1 + a * TMX_NP + ii, j = 1 + b * TMX_NP + jj;
			plan.ucol.push_back(col_of(P, i, j));
			const bool da = (ii == 0 && a > 0), db = (jj == 0 && b > 0);
			plan.udep.push_back(da ? col_of(P, i - 1, j) : -1);
			plan.udep.push_back(db ? col_of(P, i, j - 1) : -1);
			plan.udep.push_back((da && db) ? col_of(P, i - 1, j - 1) : -1);
		}
	}
	e->nunique = (int)plan.ucol.size();
	e->NUS = ((e->nunique + 63) / 64) * 64;
}

// what the launches read beside the group tables: all of it follows from the groups, the send list and the options
static void build_launch_tables(tmx_engine * e) {
	PlanHost & plan = e->plan;
	const int NR = e->cfg.n_ranks;
	// column -> its other copies: the group table inverted, for kernels that average while loading (k_hypervis<PULL>):
	// {the three other members in group order, n | me << 3 | type << 6 | (matrix index + 1) << 8}; all zero / -1: no copies
	plan.colref.assign((size_t)e->NS * 4, 0);
	for (size_t c = 0; c < (size_t)e->NS; c++) { plan.colref[c * 4] = plan.colref[c * 4 + 1] = plan.colref[c * 4 + 2] = -1; }
	for (int g = 0; g < e->ngroups; g++)
		for (int m = 0; m < plan.grp_n[g]; m++) {
			const int c = plan.grp_cols[(size_t)g * 4 + m];
			if (c < 0 || c >= e->NS) continue;
			int q = 0;
			for (int o = 0; o < 4; o++) if (o != m) plan.colref[(size_t)c * 4 + q++] = (o < plan.grp_n[g]) ? plan.grp_cols[(size_t)g * 4 + o] : -1;
			plan.colref[(size_t)c * 4 + 3] = plan.grp_n[g] | (m << 3) | (((plan.grp_type[g] >> (2 * m)) & 3) << 6) | ((plan.grp_x[g] + 1) << 8);
		}
	// element blocks of the fused hyperviscosity kernel: 5 x 5 inner elements (kernels: TMX_HB_E) per block, patch by patch
	for (int pp : e->local_patches) {
		const PatchInfo & P = e->patches[pp];
		for (int a0 = 0; a0 < P.nea; a0 += 5) for (int b0 = 0; b0 < P.neb; b0 += 5)
			plan.hvblocks.insert(plan.hvblocks.end(), { P.elem_base, P.nea, P.neb, a0, b0 });
	}
	// Boundary-first launches (north-star: "exchange overlapped with interior-element updates").  A 64-column tile (four
	// elements) is EARLY when it holds a column some other rank needs; the kernels that feed an exchange run on the early
	// tiles first, the pack + grouped send/recv starts on the exchange stream, and the remaining tiles -- three quarters
	// of a 15 x 15-element patch -- are updated while the wire is busy (produce_and_average, tmx_step.hip).  TMX_NO_SPLIT=1 switches it off.
	// The stage splits when both lists have tiles; otherwise both stay empty.
	if (NR > 1 && !plan.send_cols.empty() && !e->opt_no_split) {
		std::vector<char> early(e->NS / 64, 0);
		for (int c : plan.send_cols) early[c / 64] = 1;
		for (int t = 0; t < (int)early.size(); t++) (early[t] ? plan.quads_early : plan.quads_late).push_back(t);
		if (plan.quads_early.empty() || plan.quads_late.empty()) { plan.quads_early.clear(); plan.quads_late.clear(); }
	}
	// wire layout [peer][slab][count_peer]: element t of a peer's segment at nslab*off + slab*count + (t - off)
	plan.send_base.resize(e->nsend); plan.send_stride.resize(e->nsend); plan.ghost_base.resize(e->nghost); plan.ghost_stride.resize(e->nghost);
	for (int rk = 0; rk < NR; rk++) {
		const int so = e->send_rank_off[rk], sc = e->send_rank_off[rk + 1] - so;
		for (int t = 0; t < sc; t++) { plan.send_base[so + t] = e->nslab * so + t; plan.send_stride[so + t] = sc; }
		const int ro = e->recv_rank_off[rk], rc = e->recv_rank_off[rk + 1] - ro;
		for (int t = 0; t < rc; t++) { plan.ghost_base[ro + t] = e->nslab * ro + t; plan.ghost_stride[ro + t] = rc; }
	}
	// Columns per wavefront of the two-wavefront column kernel.  A pair (assembly + elimination wavefront) is the unit of
	// residency: 512 pairs give every SIMD of the 256 CUs one wavefront, 1024 two.  With 64 columns per pair a grid
	// such as ne30 (760 groups) loads 124 CUs twice and 132 once and the kernel runs as long as the doubly loaded ones;
	// with ceil(nunique / (512 m)) columns per pair (48 at ne30) every SIMD carries the same number of wavefronts.
	// (measured at ne30: 56 columns per wavefront = 64; 48 and 40, which would load every SIMD evenly, are 70 % SLOWER --
	// the kernel is not bound by the doubly loaded CUs; the knob stays for experiments, the default is 64)
	e->vi_cpw = (e->opt_vi_cpw >= 1 && e->opt_vi_cpw <= 64) ? e->opt_vi_cpw : 64;
	// stream columns of the column-solve scratch (upload_plan: d_ab)
	const int ngrp = (e->nunique + e->vi_cpw - 1) / e->vi_cpw + 2;
	e->vi_stream_cols = std::max(e->NUS, ngrp * 64);
	// the lane-group kernel (k_vi_group) streams 16 doubles per row and column instead of 10
	if (e->vi_group == 1 || (e->vi_group < 0 && e->nunique <= e->vi_group_max))
		e->vi_stream_cols = std::max(e->vi_stream_cols, (int)(((size_t)16 * (e->nunique + 4) + 9) / 10) + 64);
}

static int build_plan(tmx_engine * e) {
	const Nodes N(e);
	Groups groups;
	std::map<int, int> ghost_index;
	int r;
	if ((r = build_groups(e, N, groups, ghost_index))) return r;
	if ((r = build_group_tables(e, N, groups, ghost_index))) return r;
	build_unique_columns(e);
	build_launch_tables(e);
	return TMX_OK;
}

// ---------------------------------------------------------------------------------------------
// device engines: what the geometry calls left on the host becomes final, then everything goes to the device

// closed-form metric or stored arrays, the element spacing of every column, Rayleigh layer or none
static int settle_geometry(tmx_engine * e) {
	// closed-form 3-D metric only if every owned patch delivered factors that reproduce its arrays exactly
	e->metric_closed = !e->sw && !e->h_eta.empty();
	for (int lp : e->local_patches) e->metric_closed = e->metric_closed && e->patches[lp].metric_ok;
	if (e->opt_metric_stored) e->metric_closed = false;
	// per-column element spacing and local hyperviscosity scale of the column's patch
	for (int lp : e->local_patches) {
		const PatchInfo & P = e->patches[lp];
		const double da = (P.da > 0.0) ? P.da : e->cfg.element_delta_a, db = (P.db > 0.0) ? P.db : e->cfg.element_delta_a;
		const double ida = 1.0 / da, idb = 1.0 / db;
		const double nus = (e->cfg.reference_length != 0.0) ? pow(da / e->cfg.reference_length, 3.2) : 1.0;
		for (int c = P.elem_base * TMX_NQ; c < (P.elem_base + P.nea * P.neb) * TMX_NQ; c++) {
			e->h_g2d[G2_IDA * e->NS + c] = ida; e->h_g2d[G2_IDB * e->NS + c] = idb; e->h_g2d[G2_NUS * e->NS + c] = nus;
		}
	}
	int nset = 0;
	for (int lp : e->local_patches) nset += e->patches[lp].rayleigh_set ? 1 : 0;
	REQUIRE(nset == 0 || nset == (int)e->local_patches.size(), TMX_ERR_INVALID, "tmx_set_patch_rayleigh was called for %d of %d owned patches", nset, (int)e->local_patches.size());
	e->rayleigh = nset > 0;
	return TMX_OK;
}

// Node-unique state layout (tmx_unique.hip): for the configurations all of whose step kernels have the U form -- the
// nonhydrostatic set with implicit vertical dynamics, no tracers, no uniform diffusion, closed-form metric; a Rayleigh layer (its
// strength is stored per copy of a node) since round 5: the relaxation at the end of StepAfterSubCycle reads node-unique and writes
// element-major, and the next step reads that copy by copy ("unique_mixed").  Every other configuration, and every entry point other
// than tmx_step, works on the element-major layout as before.
static bool unique_layout_eligible(const tmx_engine * e) {
	return e->u.option != 0 && !e->sw && !e->fully_explicit && !e->udiff && e->nt == 0 && (!e->rayleigh || (e->u.mixed_option && e->u.tile_shape == 0)) && e->metric_closed &&
	       !e->hvis_pull && !e->hvis_block && !e->use_graph && !e->use_mfma && e->vi_mode == 0;
}

// Nothing but hipSetDevice, allocate, copy, memset and the sum of the bytes.  The ORDER and the SIZES of the allocations are those of every
// earlier version of tmx_finalize: where the large buffers lie relative to each other is an unmeasured input to bandwidth-bound kernels.
static int upload_plan(tmx_engine * e) {
	const PlanHost & plan = e->plan;
	int r;
	HIPCHK(hipSetDevice(e->device));
	size_t bytes = 0;
	const size_t NS = e->NS; const int L = e->L;
	const size_t state_bytes = (size_t)e->cfg.n_instances * e->inst_stride * sizeof(double);
	HIPCHK(hipMalloc((void **)&e->d_state, state_bytes)); bytes += state_bytes;
	HIPCHK(hipMemset(e->d_state, 0, state_bytes));
	if ((r = dev_upload(&e->d_g2d, e->h_g2d, &bytes))) return r;
	if (e->metric_closed) {
		if ((r = dev_upload(&e->d_eta, e->h_eta, &bytes))) return r;
	} else {
		if ((r = dev_upload(&e->d_g3n, e->h_g3n, &bytes))) return r;
		if ((r = dev_upload(&e->d_g3e, e->h_g3e, &bytes))) return r;
	}
	if ((r = dev_upload(&e->d_ops, e->h_ops, &bytes))) return r;
	if (e->nt > 0) {
		if ((r = dev_upload(&e->d_area, e->h_area, &bytes))) return r;
		HIPCHK(hipMalloc((void **)&e->d_w0, (size_t)(L + 1) * NS * sizeof(double))); bytes += (size_t)(L + 1) * NS * sizeof(double);
	}
	if (e->udiff) {
		// reference state in the layout of a state instance (filled by tmx_set_patch_reference_state)
		const size_t rb = (size_t)e->nslab * NS * sizeof(double);
		HIPCHK(hipMalloc((void **)&e->d_ref, rb)); HIPCHK(hipMemset(e->d_ref, 0, rb)); bytes += rb;
	}
	if (e->rayleigh) {
		if ((r = dev_upload(&e->d_ray_nu, e->h_ray_nu, &bytes))) return r;
		if ((r = dev_upload(&e->d_ray_ref, e->h_ray_ref, &bytes))) return r;
	}
	HIPCHK(hipMalloc((void **)&e->d_scratch, (size_t)(L + 4) * NS * sizeof(double))); bytes += (size_t)(L + 4) * NS * sizeof(double);
	HIPCHK(hipMemset(e->d_scratch, 0, (size_t)(L + 4) * NS * sizeof(double)));
	if ((r = dev_upload(&e->d_grp_cols, plan.grp_cols, &bytes))) return r;
	if ((r = dev_upload(&e->d_colref, plan.colref, &bytes))) return r;
	e->n_hvblocks = (int)(plan.hvblocks.size() / 5);
	if (e->n_hvblocks && (r = dev_upload(&e->d_hvblocks, plan.hvblocks, &bytes))) return r;
	if ((r = dev_upload(&e->d_grp_n, plan.grp_n, &bytes))) return r;
	if ((r = dev_upload(&e->d_grp_x, plan.grp_x, &bytes))) return r;
	if ((r = dev_upload(&e->d_grp_type, plan.grp_type, &bytes))) return r;
	if ((r = dev_upload(&e->d_xmat, plan.xmat, &bytes))) return r;
	if ((r = dev_upload(&e->d_send_cols, plan.send_cols, &bytes))) return r;
	e->split_stage = !plan.quads_early.empty();
	if (e->split_stage) {
		if ((r = dev_upload(&e->d_quads_early, plan.quads_early, &bytes)) || (r = dev_upload(&e->d_quads_late, plan.quads_late, &bytes))) return r;
		e->n_quads_early = (int)plan.quads_early.size(); e->n_quads_late = (int)plan.quads_late.size();
	}
	REQUIRE((long long)e->nslab * std::max(e->nsend, e->nghost) < 0x7fffffffLL, TMX_ERR_UNSUPPORTED, "exchange buffer exceeds 2^31 doubles");
	if ((r = dev_upload(&e->d_send_base, plan.send_base, &bytes))) return r;
	if ((r = dev_upload(&e->d_send_stride, plan.send_stride, &bytes))) return r;
	if ((r = dev_upload(&e->d_ghost_base, plan.ghost_base, &bytes))) return r;
	if ((r = dev_upload(&e->d_ghost_stride, plan.ghost_stride, &bytes))) return r;
	if ((r = dev_upload(&e->d_ucol, plan.ucol, &bytes))) return r;
	if ((r = dev_upload(&e->d_udep, plan.udep, &bytes))) return r;
	const size_t gb = (size_t)e->nslab * e->nghost_pad * sizeof(double), sb = (size_t)e->nslab * std::max(e->nsend, 1) * sizeof(double);
	HIPCHK(hipMalloc((void **)&e->d_ghost, gb)); HIPCHK(hipMemset(e->d_ghost, 0, gb)); bytes += gb;
	HIPCHK(hipMalloc((void **)&e->d_sendbuf, sb)); bytes += sb;
	const int n = TMX_FTOT * (L + 1);
	// column-solve scratch: per-wavefront U-row streams [NUS/64][n][9 + 1][64] plus a zero page (fused / pair kernels);
	// the split cross-check kernels keep the band matrix [n][9][NUS] and the right-hand sides [n][NUS] in the same buffers
	const size_t zpage = 128 * sizeof(double);      // one 16-byte slot per lane
	const size_t abb = (size_t)n * (TMX_BW + 1) * e->vi_stream_cols * sizeof(double) + zpage, rb = (size_t)n * e->NUS * sizeof(double);
	HIPCHK(hipMalloc((void **)&e->d_ab, abb)); HIPCHK(hipMemset((char *)e->d_ab + abb - zpage, 0, zpage)); bytes += abb;
	HIPCHK(hipMalloc((void **)&e->d_rhs, rb)); bytes += rb;
	// (behind the flag word: the order slots of the column solve's workgroups, one int per CU -- 16 XCC ids x 256 CU / SH / SE ids; k_vi_pair)
	HIPCHK(hipMalloc((void **)&e->d_flag, (64 + 4096) * sizeof(int))); HIPCHK(hipMemset(e->d_flag, 0, (64 + 4096) * sizeof(int)));
	if (unique_layout_eligible(e)) {
		if ((r = tmxu_build(e, &bytes))) return r;
		if (e->u.NTS > NS) {      // the block thread order pads: the level-parallel kernels' hand-over arrays are indexed by thread
			hipFree(e->d_scratch); e->d_scratch = nullptr;
			HIPCHK(hipMalloc((void **)&e->d_scratch, (size_t)(L + 4) * e->u.NTS * sizeof(double))); bytes += (size_t)(L + 4) * (e->u.NTS - NS) * sizeof(double);
			HIPCHK(hipMemset(e->d_scratch, 0, (size_t)(L + 4) * e->u.NTS * sizeof(double)));
		}
	}
	e->hbm_bytes = bytes;
	// host staging no longer needed
	for (std::vector<double> * h : { &e->h_g2d, &e->h_g3n, &e->h_g3e, &e->h_area, &e->h_ray_nu, &e->h_ray_ref }) std::vector<double>().swap(*h);
	return TMX_OK;
}

// ---------------------------------------------------------------------------------------------
// finalize: check, build, upload

extern "C" int tmx_finalize(tmx_engine * e) {
	REQUIRE(e, TMX_ERR_INVALID, "tmx_finalize: null engine");
	REQUIRE(!e->finalized, TMX_ERR_INVALID, "tmx_finalize called twice");
	REQUIRE(e->ops_set, TMX_ERR_INVALID, "tmx_set_operators must precede tmx_finalize");
	int r = ensure_layout(e);
	if (r) return r;
	for (int p = 0; p < e->cfg.n_patches; p++) {
		REQUIRE(e->patches[p].halo_set, TMX_ERR_INVALID, "halo of patch %d not set", p);
		if (e->patches[p].owner == e->cfg.rank && !plan_only(e))
			REQUIRE(e->patches[p].geom_set, TMX_ERR_INVALID, "geometry of local patch %d not set", p);
	}
	if ((r = build_plan(e))) return r;
	e->finalized = true;
	if (plan_only(e)) return TMX_OK;
	if ((r = settle_geometry(e))) return r;
	return upload_plan(e);
}

// ---------------------------------------------------------------------------------------------
// introspection of the plan

// exchange / DSS plan for host-side tests (include/tempest_mi355x.h lists the values of `what`).  Returns the number of ints written
// (or needed when out == nullptr).
extern "C" int tmx_plan_get(tmx_engine * e, int what, int * out, int cap) {
	if (!e || !e->finalized) return -1;
	const PlanHost & plan = e->plan;
	std::vector<int> v;
	if (what == 0 || what == 1) {
		const std::vector<int> & nodes = what ? plan.recv_nodes : plan.send_nodes;
		const std::vector<int> & off = what ? e->recv_rank_off : e->send_rank_off;
		for (int rk = 0; rk < e->cfg.n_ranks; rk++)
			for (int t = off[rk]; t < off[rk + 1]; t++) { v.push_back(nodes[3 * t]); v.push_back(nodes[3 * t + 1]); v.push_back(nodes[3 * t + 2]); v.push_back(rk); }
	} else if (what == 2) {
		for (int g = 0; g < e->ngroups; g++) { v.push_back(plan.grp_n[g]); for (int m = 0; m < 4; m++) v.push_back(plan.grp_cols[(size_t)g * 4 + m]); }
	} else if (what == 3) {
		v.push_back(e->NS); v.push_back(e->ncol); v.push_back(e->nunique); v.push_back(e->ngroups); v.push_back(e->nxgroups);
	} else if (what == 4) {
		v = plan.grp_x;
	} else if (what == 5) {
		v = plan.grp_type;
	} else if (what == 6) {
		v = plan.colref;
	} else if (what == 7) {
		v = plan.quads_early;
	} else if (what == 8) {
		v = plan.quads_late;
	} else if (what == 9) {
		for (const std::vector<int> * t : { &plan.send_base, &plan.send_stride, &plan.ghost_base, &plan.ghost_stride }) v.insert(v.end(), t->begin(), t->end());
	} else if (what == 10) {
		v = plan.send_cols;
	} else return -1;
	if (out) { if ((int)v.size() > cap) return -1; if (!v.empty()) memcpy(out, v.data(), v.size() * sizeof(int)); }      // (an empty table has no data pointer to hand to memcpy: found by the sanitized build)
	return (int)v.size();
}

// cross-panel covector matrices of the DSS groups: [n_cross][member m][partner q][2x2], the matrix that rotates q's
// (U,V) into the frame of m's patch (identity where q == m or both lie on one panel)
extern "C" int tmx_plan_get_matrices(tmx_engine * e, double * out, int cap) {
	if (!e || !e->finalized) return -1;
	const PlanHost & plan = e->plan;
	if (out) { if ((int)plan.xmat.size() > cap) return -1; if (!plan.xmat.empty()) memcpy(out, plan.xmat.data(), plan.xmat.size() * sizeof(double)); }
	return (int)plan.xmat.size();
}

// Host-side tables of the node-unique layout for the tile shape given, built on the spot (works on plan-only engines: no device),
// for the CPU tests of that logic.  what = 0: (NU, NUS, NTS, slots, groups left to the DSS kernel, of them without remote member,
// early tiles, late tiles); 1 t_dcol; 2 t_ucol; 3 t_sdst; 4 t_sred; 5 gsrc; 6 gdst; 7 gn; 8 slot_ucol; 9 send_slots; 10 u_rep;
// 11 ucol_of_dcol; 12 per-tile info.  Returns the number of ints written (needed, when out == NULL), -1 on error.
extern "C" int tmx_debug_unique_tables(tmx_engine * e, int tile_shape, int what, int * out, int cap) {
	if (!e || !e->finalized || tile_shape < 0 || tile_shape > 4) return -1;
	UniqueLayout keep = e->u;
	e->u = UniqueLayout(); e->u.tile_shape = tile_shape;
	UniqueTables T;
	const int r = tmxu_tables(e, T);
	const UniqueLayout u = e->u;
	e->u = keep;
	if (r) return -1;
	std::vector<int> v;
	switch (what) {
		case 0: v = { u.NU, u.NUS, u.NTS, u.nslots, u.ngroups, u.ngroups_local, u.n_early, u.n_late, u.b_ngroups, u.b_ngroups_local, u.nblocks, u.nb_early, u.nb_late }; break;
		case 13: v = T.b_sdst; break; case 14: v = T.b_sred; break; case 15: v = T.blk_info; break; case 16: v = T.b_gsrc; break; case 17: v = T.b_gdst; break; case 18: v = T.b_gn; break;
		case 19: v = T.blks_early; break; case 20: v = T.blks_late; break;
		case 1: v = T.t_dcol; break; case 2: v = T.t_ucol; break; case 3: v = T.t_sdst; break; case 4: v = T.t_sred; break;
		case 5: v = T.gsrc; break; case 6: v = T.gdst; break; case 7: v = T.gn; break; case 8: v = T.slot_ucol; break;
		case 9: v = T.send_slots; break; case 10: v = T.u_rep; break; case 11: v = T.ucol_of_dcol; break; case 12: v = T.tinfo; break;
		default: return -1;
	}
	if (out) { if ((int)v.size() > cap) return -1; if (!v.empty()) memcpy(out, v.data(), v.size() * sizeof(int)); }
	return (int)v.size();
}
