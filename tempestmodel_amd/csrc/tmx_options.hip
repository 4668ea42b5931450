// tmx_options.hip -- the engine's options: ONE table row per option says everything about it; tmx_set_option, tmx_get_option,
// tmx_options_report and tmx_options_from_environment are loops over the table.
#include "tmx_hostshared.h"
#include <climits>

// Options that change how (never what) the engine computes -- the one exception, "contraction_mfma", is named as such -- by name.
// The library reads NO environment variable on its own: a stray TMX_* in a job script cannot change a run.  Test and bench plumbing
// that wants the historical variables calls tmx_options_from_environment, which turns them into these options, prints ONE line
// naming what it applied, and leaves them queryable (tmx_get_option, tmx_options_report).
struct Values { int lo, hi; std::vector<int> one_of; };      // the values accepted: a range, or (one_of not empty) a short list
struct Refused { int lo, hi; };                              // what the production flavour refuses of them: this range, the option's default excepted
// how the variable's text becomes the value: its integer; 1 when the variable exists at all (its presence alone was the switch); 1 when the integer
// is not 0; 1 when the text is the word given; the integer / 10
enum EnvMode { AS_INT, AS_PRESENT, AS_NONZERO, AS_WORD, AS_TENTH };
struct EnvDecode { EnvMode mode; const char * word = nullptr; };
struct OptionDef {
	const char * name; const char * env;
	bool before_finalize;                                    // settable only until tmx_finalize
	int * (*slot)(tmx_engine *);                             // its field of the engine (the launchers read the fields, not this table)
	Values ok; Refused production; EnvDecode decode;
	const char * help;
};
#define F(FIELD_) [](tmx_engine * e) -> int * { return &e->FIELD_; }
#define R(LO_, HI_) Values{ LO_, HI_, {} }
#define ANY R(INT_MIN, INT_MAX)
#define ONE_OF(...) Values{ INT_MIN, INT_MAX, { __VA_ARGS__ } }
// production flavour: every accepted value; all but a range; or the default alone -- an archived experiment or a cross-check kernel that only
// the experiments flavour of the library holds (-DTMX_EXPERIMENTS, libtempest_mi355x_exp.so)
#define ALL Refused{ 1, 0 }
#define BUT(LO_, HI_) Refused{ LO_, HI_ }
#define DEFAULT_ONLY Refused{ INT_MIN, INT_MAX }
static const bool BEFORE_FINALIZE = true, ANY_TIME = false;
// (tmx_options_report and the from_environment line print in this order)
static const OptionDef g_options[] = {
	{ "unique_layout", "TMX_UNIQUE", BEFORE_FINALIZE, F(u.option), R(-1, 1), ALL, { AS_NONZERO }, "node-unique state layout inside tmx_step: -1 default (= 1), 0 off, 1 on where eligible" },
	{ "unique_tile_shape", "TMX_UNIQUE_TILE", BEFORE_FINALIZE, F(u.tile_shape), R(0, 4), BUT(3, 4), { AS_INT }, "elements of a wavefront on that layout: 0 (default, measured fastest) the element-major order = 1 x 4 strips that wrap around patch rows, 1 = 2 x 2 blocks, 2 = strips that stay inside a patch row; experiments flavour only: 3 = a generalised Hilbert curve through every patch, 4 = 4 x 4 element blocks of 1 x 4 strips" },
	{ "unique_blocks", "TMX_UNIQUE_BLOCKS", ANY_TIME, F(u.block_option), R(-1, 3), DEFAULT_ONLY, { AS_INT }, "archived experiment (round 6: the DSS loses 0.05 ms per step, the producers pay 0.10): block kernels on that layout -- a workgroup of four wavefronts averages the seams between them through LDS, the DSS kernel finishes fewer nodes: -1 (default) on with unique_tile_shape 4, 0 off, 1 on with any thread order" },
	{ "unique_xcd_order", "TMX_UNIQUE_XCD", BEFORE_FINALIZE, F(u.xcd_order), R(0, 1), DEFAULT_ONLY, { AS_INT }, "A/B switch, experiments flavour only: 1 (default): every XCD sweeps a contiguous range of tiles" },
	{ "unique_mixed", "TMX_UNIQUE_MIXED", BEFORE_FINALIZE, F(u.mixed_option), R(0, 1), ALL, { AS_INT }, "1 (default): the explicit stages read a live-in element-major instance copy by copy (no check, no conversion); 0: check the copies, convert or run the step element-major" },
	{ "unique_prefix", "TMX_UNIQUE_PREFIX", ANY_TIME, F(u.prefix_option), R(0, 1), ALL, { AS_INT }, "1 (default): an explicit stage also stores the leading partial sum of a later stage's combination over the instances both read (ARS343: the fourth stage reads 3 instances instead of 7); 0: every stage reads all its terms" },
	{ "share_copies", "TMX_SHARE_COPIES", ANY_TIME, F(share_copies), R(0, 1), ALL, { AS_INT }, "1 (default): stage copies that stay identical to their source share its slot instead of being made" },
	{ "xcd_vertical", "TMX_XCD_VERTICAL", ANY_TIME, F(xcd_vertical), R(0, 1), DEFAULT_ONLY, { AS_NONZERO }, "A/B switch, experiments flavour only: 1 (default): level blocks of a column tile on one XCD in the vertical stencil kernels" },
	{ "vi_carry", "TMX_VI_CARRY", ANY_TIME, F(vi_carry), R(-1, 1), DEFAULT_ONLY, { AS_NONZERO }, "column solve: carry shared sub-expressions between block rows (1)" },
	{ "vi_pair", "TMX_VI_PAIR", ANY_TIME, F(vi_pair), ANY, BUT(0, 0), { AS_NONZERO }, "column solve: two-wavefront kernel (-1 auto, 0 one-wavefront kernel, 1 on)" },
	{ "vi_group", "TMX_VI_GROUP", BEFORE_FINALIZE, F(vi_group), R(-1, 1), ALL, { AS_NONZERO }, "column solve: one column per 16-lane group (-1 auto: up to vi_group_max unique columns, 0, 1)" },
	{ "vi_group_max", "TMX_VI_GROUP_MAX", BEFORE_FINALIZE, F(vi_group_max), R(0, INT_MAX), ALL, { AS_INT }, "largest rank share (unique columns) served by the lane-group kernel (6400)" },
	{ "vi_pair_workgroup", "TMX_VI_PAIR_WG", ANY_TIME, F(vi_pair_wg), R(0, 2), ALL, { AS_INT }, "pairs per workgroup of the two-wavefront kernel (0 auto)" },
	{ "vi_ring_depth", "TMX_VI_RING_DEPTH", ANY_TIME, F(vi_ring_depth), ONE_OF(0, 2, 3), ALL, { AS_INT }, "block rows in the LDS ring between assembly and elimination: 0 auto (3, or 2 where only that fits two workgroups per CU: 37 to 82 levels with two pairs per workgroup), 2, 3" },
	{ "vi_producers", "TMX_VI_PRODUCERS", ANY_TIME, F(vi_producers), R(0, 2), ALL, { AS_INT }, "assembly wavefronts per column group of that kernel: 0 auto (2 on grids that leave every wavefront a SIMD of its own), 1, 2" },
	{ "vi_split_back", "TMX_VI_SPLIT_BACK", ANY_TIME, F(vi_split_back), ANY, DEFAULT_ONLY, { AS_INT }, "back substitution as a launch of its own (0)" },
	{ "vi_back_sub", "TMX_VI_BACK_SUB", ANY_TIME, F(vi_back_sub), ONE_OF(1, 2, 4), DEFAULT_ONLY, { AS_INT }, "wavefronts per column group of that launch (1)" },
	{ "vi_stagger", "TMX_VI_STAGGER_NS", ANY_TIME, F(vi_stagger), R(0, INT_MAX), DEFAULT_ONLY, { AS_TENTH }, "A/B switch, experiments flavour only: staggered workgroup starts, window in units of 10 ns (0)" },
	{ "vi_split_kernels", "TMX_VI_MODE", BEFORE_FINALIZE, F(vi_mode), ANY, DEFAULT_ONLY, { AS_WORD, "split" }, "1: assemble + solve as two kernels (cross-check path)" },
	{ "vi_sparse", "TMX_VI_SPARSE", ANY_TIME, F(opt_vi_sparse), R(0, 1), DEFAULT_ONLY, { AS_INT }, "1 (default): U-row entries that are zero in all 64 columns are not stored" },
	{ "vi_columns_per_wavefront", "TMX_VI_CPW", BEFORE_FINALIZE, F(opt_vi_cpw), R(0, 64), ALL, { AS_INT }, "columns per wavefront of the two-wavefront kernel (0 = 64)" },
	{ "contraction_mfma", "TMX_MFMA", BEFORE_FINALIZE, F(use_mfma), R(0, 1), ALL, { AS_NONZERO }, "1: the 4 x 4 contractions of the fused explicit kernel on the matrix unit -- NOT bit-exact (1e-15 per call, W 1.5e-10 after 100 steps)" },
	{ "step_graph", "TMX_GRAPH", BEFORE_FINALIZE, F(use_graph), R(0, 1), ALL, { AS_NONZERO }, "1: single-rank steps replayed from a captured hipGraph" },
	{ "p2p_timeout_s", "TMX_P2P_TIMEOUT_S", ANY_TIME, F(p2p_timeout_s), R(0, INT_MAX), ALL, { AS_INT }, "peer-to-peer halo: seconds a neighbour's message may take (600; 0 = for ever)" },
	{ "hvis_pull", "TMX_HVIS_PULL", BEFORE_FINALIZE, F(hvis_pull), ANY, DEFAULT_ONLY, { AS_INT }, "archived experiment: DSS pulled into the second hyperviscosity pass" },
	{ "hvis_block", "TMX_HVIS_BLOCK", BEFORE_FINALIZE, F(hvis_block), ANY, DEFAULT_ONLY, { AS_INT }, "archived experiment: hyperviscosity passes fused with the in-patch DSS" },
	{ "split_stage_off", "TMX_NO_SPLIT", BEFORE_FINALIZE, F(opt_no_split), ANY, ALL, { AS_PRESENT }, "1: no boundary-first stages on several ranks" },
	{ "metric_stored", "TMX_METRIC", BEFORE_FINALIZE, F(opt_metric_stored), ANY, ALL, { AS_WORD, "stored" }, "1: stream the stored 3-D metric arrays even where the closed form is verified" },
	{ "tracer_lincomb_pass", "TMX_TRACER_LINCOMB_PASS", ANY_TIME, F(opt_tracer_lincomb_pass), ANY, DEFAULT_ONLY, { AS_PRESENT }, "A/B switch, experiments flavour only: 1: tracer stage combination by a separate pass (A/B)" },
	{ "udv_separate", "TMX_UDV_SEPARATE", ANY_TIME, F(opt_udv_separate), ANY, DEFAULT_ONLY, { AS_PRESENT }, "A/B switch, experiments flavour only: 1: vertical diffusion of U,V as a pass of its own (A/B)" },
	{ "vx_fused", "TMX_VX_FUSED", ANY_TIME, F(opt_vx_fused), ANY, DEFAULT_ONLY, { AS_PRESENT }, "1: V.StepExplicit's U,V update inside the explicitly-treated-terms kernel (A/B)" },
	{ "debug_skip_exchange", "TMX_DEBUG_SKIP_EXCHANGE", ANY_TIME, F(opt_skip_exchange), ANY, DEFAULT_ONLY, { AS_PRESENT }, "TIMING AID, WRONG RESULTS at rank boundaries: a lone rank engine of an N-rank layout with the wire left out" },
	{ "exchange_overlap_off", "TMX_NO_EXCHANGE_OVERLAP", BEFORE_FINALIZE, F(opt_no_exchange_overlap), ANY, ALL, { AS_PRESENT }, "1: the exchange runs on the engine's stream" },
	{ "kessler_column", "TMX_KESSLER_COLUMN", ANY_TIME, F(opt_kessler_column), ANY, ALL, { AS_INT }, "1: one-lane-per-column Kessler kernel (cross-check)" },
	{ "dcmip_lds", "TMX_DCMIP_LDS", ANY_TIME, F(opt_dcmip_lds), ANY, ALL, { AS_INT }, "1: DCMIP2016 physics with its Thomas coefficients in LDS where they fit (A/B; one workgroup per CU at L30: slower)" },
	{ "vt_column", "TMX_VT_COLUMN", ANY_TIME, F(opt_vt_column), ANY, ALL, { AS_PRESENT }, "1: one-lane-per-column explicit tracer update (cross-check)" },
	{ "vt_explicit_v1", "TMX_VT_EXPLICIT_V1", ANY_TIME, F(opt_vt_explicit_v1), ANY, DEFAULT_ONLY, { AS_PRESENT }, "1: level-parallel explicit tracer update without LDS staging (cross-check)" },
	{ "vt_explicit_walk", "TMX_VT_WALK", ANY_TIME, F(opt_vt_walk), ANY, BUT(1, INT_MAX), { AS_INT }, "explicit tracer update: -1000 (default) a sliding register window over column segments, their number chosen from the grid size; -n = n segments; 0 = the LDS-tiled level-parallel kernel; 4, 5, 6, 8, 10 = that many levels per thread held in registers (experiments build)" },
	{ "vite_walk", "TMX_VITE_WALK", ANY_TIME, F(opt_vite_walk), ANY, ALL, { AS_INT }, "explicitly evaluated implicit terms (StepImplicitTermsExplicitly): -1000 (default) a sliding register window over column segments, their number chosen from the grid size; -n = n segments; 0 = the level-parallel kernel" },
	{ "vx_walk", "TMX_VX_WALK", ANY_TIME, F(opt_vx_walk), ANY, ALL, { AS_INT }, "V.StepExplicit's U,V update: -1000 (default) a sliding register window over column segments, their number chosen from the grid size; -n = n segments; 0 = the level-parallel kernel" },
	{ "vt_lanes", "TMX_VT_LANES", ANY_TIME, F(opt_vt_lanes), ONE_OF(8, 16, 32, 64), DEFAULT_ONLY, { AS_INT }, "A/B switch, experiments flavour only: columns per workgroup of the implicit tracer kernel's one-row-lane form, \"vt_rows\" = 0 (16)" },
	{ "vt_lw8", "TMX_VT_LW8", ANY_TIME, F(opt_vt_lw8), R(-1, 1), DEFAULT_ONLY, { AS_INT }, "A/B switch, experiments flavour only: row-parallel tracer kernel: 8 columns per workgroup (-1 auto)" },
	{ "vt_row_lanes", "TMX_VT_NR", ANY_TIME, F(opt_vt_nr), ONE_OF(0, 4, 8, 16, 32), DEFAULT_ONLY, { AS_INT }, "A/B switch, experiments flavour only: row lanes of that kernel (0 auto)" },
	{ "vt_rows", "TMX_VT_ROWS", ANY_TIME, F(opt_vt_rows), R(0, 1), ALL, { AS_INT }, "1 (default): implicit tracer update with several row lanes per column; 0: the same kernel with one row lane per column, the serial order (cross-check)" },
	{ "lu_fma", "TMX_LU_FMA", ANY_TIME, F(lu_fma), R(0, 1), ALL, { AS_INT }, "band LU of the column solves: 1 (default) updates a - l u as ONE rounding (fused multiply-add: a reference linked to OpenBLAS, or to MKL on its FMA code paths), 0 = multiply and subtract rounded separately (a BLAS without fused multiply-adds); tmx_lu_flavour_from_dgbsv asks the caller's own LAPACK" },
	{ "h_walk_udiff", "TMX_H_WALK_UDIFF", ANY_TIME, F(opt_h_walk_udiff), R(0, 2), ALL, { AS_INT }, "uniform-diffusion configurations: the explicit stage's walk applies the horizontal uniform diffusion to its results in registers (1) and V.StepExplicit's U,V part behind it (2, default); 0 = k_uniform_diffusion and k_v_explicit as passes of their own (bit-identical)" },
	{ "hv_walk", "TMX_HV_WALK", ANY_TIME, F(opt_hv_walk), R(-64, 1), ALL, { AS_INT }, "hyperviscosity pass on the node-unique layout: 1 (default) a wavefront walks a segment of levels (k_hv_walk; -n: n segments per column), 0 = the level-parallel k_hypervis (bit-identical)" },
	{ "h_walk", "TMX_H_WALK", ANY_TIME, F(opt_h_walk), ANY, ALL, { AS_INT }, "explicit stage on the node-unique layout: -1000 (default) a wavefront walks a column segment with a sliding register window, segments per column from the grid size; -n = n segments; 0 = the level-parallel kernel + k_h_w_update" },
};

static const OptionDef * find_option(const char * name) {
	for (const OptionDef & d : g_options) if (strcmp(name, d.name) == 0) return &d;
	return nullptr;
}
// the default of an option: what a default-constructed engine holds
static int option_default(const OptionDef & d) { static tmx_engine fresh; return *d.slot(&fresh); }
static std::string describe(const Values & v) {
	std::string s;
	if (!v.one_of.empty()) { for (int x : v.one_of) s += (s.empty() ? "one of " : ", ") + std::to_string(x); return s; }
	if (v.lo == INT_MIN && v.hi == INT_MAX) return "any integer";
	if (v.hi == INT_MAX) return "at least " + std::to_string(v.lo);
	return std::to_string(v.lo) + " .. " + std::to_string(v.hi);
}

// unknown name, then too late, then experiments-only, then out of range: the order decides which error a caller sees
extern "C" int tmx_set_option(tmx_engine * e, const char * name, double value) {
	REQUIRE(e && name, TMX_ERR_INVALID, "tmx_set_option: null argument");
	const OptionDef * d = find_option(name);
	REQUIRE(d, TMX_ERR_INVALID, "tmx_set_option: unknown option '%s'", name);
	REQUIRE(!(d->before_finalize && e->finalized), TMX_ERR_INVALID, "tmx_set_option(%s) after tmx_finalize", name);
	const int iv = (int)value;
	REQUIRE(TMX_EXP || iv < d->production.lo || iv > d->production.hi || iv == option_default(*d), TMX_ERR_UNSUPPORTED,
		"tmx_set_option(%s = %d): an archived experiment / cross-check kernel, compiled into the experiments flavour of the library only (libtempest_mi355x_exp.so)", name, iv);
	const Values & ok = d->ok;
	REQUIRE(iv >= ok.lo && iv <= ok.hi && (ok.one_of.empty() || std::find(ok.one_of.begin(), ok.one_of.end(), iv) != ok.one_of.end()), TMX_ERR_INVALID,
		"tmx_set_option(%s = %d): accepted is %s", name, iv, describe(ok).c_str());
	*d->slot(e) = iv;
	return TMX_OK;
}
extern "C" int tmx_get_option(tmx_engine * e, const char * name, double * value) {
	REQUIRE(e && name && value, TMX_ERR_INVALID, "tmx_get_option: null argument");
	const OptionDef * d = find_option(name);
	REQUIRE(d, TMX_ERR_INVALID, "tmx_get_option: unknown option '%s'", name);
	*value = *d->slot(e);
	return TMX_OK;
}
// "name=value" of every option, one per line, defaults included; returns the length needed (buf may be null)
extern "C" int tmx_options_report(tmx_engine * e, char * buf, int cap) {
	if (!e) return -1;
	std::string out;
	for (const OptionDef & d : g_options) out += std::string(d.name) + "=" + std::to_string(*d.slot(e)) + "\n";
	if (!e->env_applied.empty()) { out += "from_environment="; for (const std::string & v : e->env_applied) out += v + " "; out += "\n"; }
	if (buf && cap > 0) { strncpy(buf, out.c_str(), (size_t)cap - 1); buf[cap - 1] = 0; }
	return (int)out.size() + 1;
}
// The historical TMX_* variables -> options (test / bench plumbing calls this right after tmx_create; the library never does).
// Returns the number of variables applied and says so on stderr, ONE line, unless TMX_QUIET is set.
extern "C" int tmx_options_from_environment(tmx_engine * e) {
	REQUIRE(e, TMX_ERR_INVALID, "tmx_options_from_environment: null engine");
	int n = 0;
	std::string refused;
	for (const OptionDef & d : g_options) {
		const char * ev = getenv(d.env);
		if (!ev) continue;
		int v = atoi(ev);
		switch (d.decode.mode) {
			case AS_INT: break;
			case AS_PRESENT: v = 1; break;
			case AS_NONZERO: v = v ? 1 : 0; break;
			case AS_WORD: v = (strcmp(ev, d.decode.word) == 0) ? 1 : 0; break;
			case AS_TENTH: v = v / 10; break;
		}
		if (d.before_finalize && e->finalized) continue;
		if (tmx_set_option(e, d.name, v) != TMX_OK) { refused += std::string(" ") + d.env + "=" + ev; continue; }
		e->env_applied.push_back(std::string(d.env) + "=" + ev);
		n++;
	}
	if (n && !getenv("TMX_QUIET")) {
		std::string l = "tempest_mi355x: options taken from the environment:";
		for (const std::string & v : e->env_applied) l += " " + v;
		fprintf(stderr, "%s\n", l.c_str());
	}
	// a variable that would have changed the run and cannot: an error, not a silent default
	REQUIRE(refused.empty(), TMX_ERR_UNSUPPORTED, "tmx_options_from_environment: refused by this build of the library (out of range, or an experiments-only option):%s", refused.c_str());
	return n;
}
