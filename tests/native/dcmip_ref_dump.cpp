// tests/native/dcmip_ref_dump.cpp -- TEST INFRASTRUCTURE ONLY (built by tests/golden/make_golden_dcmip.py in a temporary
// directory, never by build()).  Dumps what DCMIPPhysics::Perform (test/dcmip2016/DCMIPPhysics.cpp:156-409, around
// interface/dcmip_physics_z_v1.f90) does to the reference's own DCMIP2016 tropical-cyclone and moist-baroclinic-wave states:
//
//   --case tc | bw      TropicalCycloneTest (test 2, 3 tracers) | BaroclinicWaveUMJSTest (test 1, 5 tracers)
//   --mode percall      geometry (the records golden_util.grid_from_fixture reads), then for each starting state (stock; after
//                       --warm ARS343 steps each followed by Perform(pbl 1, prec 1); a moistened, wind-boosted copy of that one
//                       with --moisten > 0) the state before and after Perform for every (pbl, prec) in {0,1}^2 and test 3,
//                       PRECT of each call
//   --mode steps        the state after each of --steps ARS343 steps, each followed by Perform(--pbl, --prec), from the
//                       state after the same --warm steps
//
// Call sites mirrored (not copied): the two tests' main (TropicalCycloneTest.cpp:225-262, BaroclinicWaveUMJSTest.cpp:244-290),
// Model::Go's step loop with its WorkflowProcess calls (src/atm/Model.cpp:430-481).  The Fortran halves are compiled where they
// lie with amdflang -O3 (as oracle/Makefile does for Kessler).
#define main tmx_unused_tc_main
#include "TropicalCycloneTest.cpp"
#undef main
#define main tmx_unused_bw_main
#include "BaroclinicWaveUMJSTest.cpp"
#undef main
#include "DCMIPPhysics.h"

#include "GridPatchGLL.h"
#include "GridPatchCSGLL.h"
#include "CubedSphereTrans.h"
#include "LinearColumnOperatorFEM.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct TmxdWriter {
	FILE * fp;
	TmxdWriter() : fp(NULL) {}
	void open(const std::string & path) {
		fp = fopen(path.c_str(), "wb");
		if (!fp) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
		fwrite("TMXD0001", 1, 8, fp);
	}
	void close() { if (fp) fclose(fp); fp = NULL; }
	void rec(const std::string & name, int dtype, const std::vector<size_t> & dims, const void * data) {
		if (!fp) return;
		unsigned int nl = name.size();
		fwrite(&nl, 4, 1, fp);
		fwrite(name.data(), 1, nl, fp);
		unsigned int dt = dtype, nd = dims.size();
		fwrite(&dt, 4, 1, fp);
		fwrite(&nd, 4, 1, fp);
		size_t tot = 1;
		for (size_t d = 0; d < dims.size(); d++) {
			unsigned long long v = dims[d];
			fwrite(&v, 8, 1, fp);
			tot *= dims[d];
		}
		fwrite(data, (dtype == 0) ? 8 : 4, tot, fp);
	}
	void f64(const std::string & name, const std::vector<size_t> & dims, const double * p) { rec(name, 0, dims, p); }
	void i32(const std::string & name, const std::vector<size_t> & dims, const int * p) { rec(name, 1, dims, p); }
	void scalar(const std::string & name, double v) { std::vector<size_t> d; d.push_back(1); f64(name, d, &v); }
	void iscalar(const std::string & name, int v) { std::vector<size_t> d; d.push_back(1); i32(name, d, &v); }
};

static std::vector<size_t> D1(size_t a) { std::vector<size_t> d; d.push_back(a); return d; }
static std::vector<size_t> D2(size_t a, size_t b) { std::vector<size_t> d = D1(a); d.push_back(b); return d; }
static std::vector<size_t> D3(size_t a, size_t b, size_t c) { std::vector<size_t> d = D2(a,b); d.push_back(c); return d; }
static std::vector<size_t> D4(size_t a, size_t b, size_t c, size_t e) { std::vector<size_t> d = D3(a,b,c); d.push_back(e); return d; }

static void dump2(TmxdWriter & w, const std::string & n, const DataArray2D<double> & a) {
	w.f64(n, D2(a.GetRows(), a.GetColumns()), &(a[0][0]));
}
static void dump3(TmxdWriter & w, const std::string & n, const DataArray3D<double> & a) {
	w.f64(n, D3(a.GetSize(0), a.GetSize(1), a.GetSize(2)), &(a[0][0][0]));
}
static void dump4(TmxdWriter & w, const std::string & n, const DataArray4D<double> & a) {
	w.f64(n, D4(a.GetSize(0), a.GetSize(1), a.GetSize(2), a.GetSize(3)), &(a[0][0][0][0]));
}

static void dumpOp(TmxdWriter & w, const std::string & n, const LinearColumnOperator & op) {
	const DataArray2D<double> & c = op.GetCoeffs();
	dump2(w, "op/" + n + "/coeff", c);
	std::vector<int> b(c.GetRows()), e(c.GetRows());
	for (size_t k = 0; k < c.GetRows(); k++) { b[k] = op.GetIxBegin()[k]; e[k] = op.GetIxEnd()[k]; }
	w.i32("op/" + n + "/begin", D1(b.size()), &b[0]);
	w.i32("op/" + n + "/end", D1(e.size()), &e[0]);
}

static std::string pname(int p) { char b[32]; snprintf(b, 32, "p%d/", p); return std::string(b); }

///////////////////////////////////////////////////////////////////////////////

static void dumpState(TmxdWriter & w, GridGLL * pGrid, const std::string & tag, int ix) {
	for (int n = 0; n < pGrid->GetActivePatchCount(); n++) {
		GridPatch * pPatch = pGrid->GetActivePatch(n);
		int p = pPatch->GetPatchIndex();
		dump4(w, "state/" + tag + "/" + pname(p) + "node", pPatch->GetDataState(ix, DataLocation_Node));
		dump4(w, "state/" + tag + "/" + pname(p) + "redge", pPatch->GetDataState(ix, DataLocation_REdge));
		if (pPatch->GetDataTracers(ix).GetSize(0) > 0)
			dump4(w, "state/" + tag + "/" + pname(p) + "tracers", pPatch->GetDataTracers(ix));
	}
}

static void dumpGeometry(TmxdWriter & w, Model & model, GridGLL * pGrid) {
	const PhysicalConstants & phys = model.GetPhysicalConstants();
	w.scalar("phys/earth_radius", phys.GetEarthRadius());
	w.scalar("phys/g", phys.GetG());
	w.scalar("phys/omega", phys.GetOmega());
	w.scalar("phys/alpha", phys.GetAlpha());
	w.scalar("phys/Rd", phys.GetR());
	w.scalar("phys/cp", phys.GetCp());
	w.scalar("phys/cv", phys.GetCv());
	w.scalar("phys/p0", phys.GetP0());
	w.scalar("grid/ztop", pGrid->GetZtop());
	w.scalar("grid/reference_length", pGrid->GetReferenceLength());
	w.iscalar("grid/has_rayleigh", pGrid->HasRayleighFriction() ? 1 : 0);
	w.iscalar("grid/has_uniform_diffusion", pGrid->HasUniformDiffusion() ? 1 : 0);

	int L = pGrid->GetRElements();
	w.f64("grid/reta_levels", D1(L), &(pGrid->GetREtaLevels()[0]));
	w.f64("grid/reta_interfaces", D1(L+1), &(pGrid->GetREtaInterfaces()[0]));
	w.f64("grid/reta_levels_normarea", D1(L), &(pGrid->GetREtaLevelsNormArea()[0]));
	w.f64("grid/reta_interfaces_normarea", D1(L+1), &(pGrid->GetREtaInterfacesNormArea()[0]));

	dump2(w, "op/dx_basis_1d", pGrid->GetDxBasis1D());
	dump2(w, "op/stiffness_1d", pGrid->GetStiffness1D());
	w.f64("op/gll_weights_1d", D1(pGrid->GetGLLWeights1D().GetRows()), &(pGrid->GetGLLWeights1D()[0]));

	dumpOp(w, "interp_node_to_redge", pGrid->GetOpInterpNodeToREdge());
	dumpOp(w, "interp_redge_to_node", pGrid->GetOpInterpREdgeToNode());
	dumpOp(w, "diff_node_to_node", pGrid->GetOpDiffNodeToNode());
	dumpOp(w, "diff_node_to_redge", pGrid->GetOpDiffNodeToREdge());
	dumpOp(w, "diff_redge_to_node", pGrid->GetOpDiffREdgeToNode());
	dumpOp(w, "diff_redge_to_redge", pGrid->GetOpDiffREdgeToREdge());
	dumpOp(w, "diffdiff_node_to_node", pGrid->GetOpDiffDiffNodeToNode());
	dumpOp(w, "diffdiff_redge_to_redge", pGrid->GetOpDiffDiffREdgeToREdge());
	dumpOp(w, "penalty_left", pGrid->GetOpPenaltyNodeToNode().GetLeftOp());
	dumpOp(w, "penalty_right", pGrid->GetOpPenaltyNodeToNode().GetRightOp());

	for (int n = 0; n < pGrid->GetActivePatchCount(); n++) {
		GridPatchGLL * pPatch = dynamic_cast<GridPatchGLL*>(pGrid->GetActivePatch(n));
		const PatchBox & box = pPatch->GetPatchBox();
		int p = pPatch->GetPatchIndex();
		std::string pn = pname(p);
		int ibox[8] = {
			box.GetPanel(), box.GetHaloElements(),
			box.GetAGlobalInteriorBegin(), box.GetAGlobalInteriorEnd(),
			box.GetBGlobalInteriorBegin(), box.GetBGlobalInteriorEnd(),
			box.GetATotalWidth(), box.GetBTotalWidth()};
		w.i32(pn + "box", D1(8), ibox);
		int inb[8];
		for (int d = 0; d < 8; d++) inb[d] = pPatch->GetNeighborPanel((Direction)d);
		w.i32(pn + "neighbor_panels", D1(8), inb);
		w.scalar(pn + "element_delta_a", pPatch->GetElementDeltaA());
		w.scalar(pn + "element_delta_b", pPatch->GetElementDeltaB());
		w.f64(pn + "a_nodes", D1(pPatch->GetANodes().GetRows()), &(pPatch->GetANodes()[0]));
		w.f64(pn + "b_nodes", D1(pPatch->GetBNodes().GetRows()), &(pPatch->GetBNodes()[0]));
		dump2(w, pn + "lon", pPatch->GetLongitude());
		dump2(w, pn + "lat", pPatch->GetLatitude());
		dump2(w, pn + "jacobian2d", pPatch->GetJacobian2D());
		dump3(w, pn + "contra_metric_2d_a", pPatch->GetContraMetric2DA());
		dump3(w, pn + "contra_metric_2d_b", pPatch->GetContraMetric2DB());
		dump3(w, pn + "jacobian", pPatch->GetJacobian());
		dump3(w, pn + "jacobian_redge", pPatch->GetJacobianREdge());
		dump4(w, pn + "contra_metric_a", pPatch->GetContraMetricA());
		dump4(w, pn + "contra_metric_b", pPatch->GetContraMetricB());
		dump4(w, pn + "contra_metric_xi", pPatch->GetContraMetricXi());
		dump4(w, pn + "contra_metric_a_redge", pPatch->GetContraMetricAREdge());
		dump4(w, pn + "contra_metric_b_redge", pPatch->GetContraMetricBREdge());
		dump4(w, pn + "contra_metric_xi_redge", pPatch->GetContraMetricXiREdge());
		dump4(w, pn + "deriv_r_node", pPatch->GetDerivRNode());
		dump4(w, pn + "deriv_r_redge", pPatch->GetDerivRREdge());
		dump3(w, pn + "element_area_node", pPatch->GetElementAreaNode());
		dump3(w, pn + "element_area_redge", pPatch->GetElementAreaREdge());
		dump2(w, pn + "topography", pPatch->GetTopography());
		dump3(w, pn + "topography_deriv", pPatch->GetTopographyDeriv());
		dump2(w, pn + "coriolis_f", pPatch->GetCoriolisF());
		dump3(w, pn + "z_levels", pPatch->GetZLevels());
		dump3(w, pn + "z_interfaces", pPatch->GetZInterfaces());
		dump4(w, pn + "ref_node", pPatch->GetReferenceState(DataLocation_Node));
		dump4(w, pn + "ref_redge", pPatch->GetReferenceState(DataLocation_REdge));
		if (pGrid->GetModel().GetEquationSet().GetTracers() > 0) dump4(w, pn + "ref_tracers", pPatch->GetReferenceTracers());
		if (pGrid->HasRayleighFriction()) {
			dump3(w, pn + "rayleigh_node", pPatch->GetRayleighStrength(DataLocation_Node));
			dump3(w, pn + "rayleigh_redge", pPatch->GetRayleighStrength(DataLocation_REdge));
		}
	}
}

// Probe the reference's covector panel transform with unit vectors at every halo node of every
// patch edge that borders a different panel (same call TransformHaloVelocities makes,
// GridPatchCSGLL.cpp:1783-1924) and record the 2x2 matrices.
static void dumpHaloTransforms(TmxdWriter & w, GridGLL * pGrid) {
	for (int n = 0; n < pGrid->GetActivePatchCount(); n++) {
		GridPatchGLL * pPatch = dynamic_cast<GridPatchGLL*>(pGrid->GetActivePatch(n));
		const PatchBox & box = pPatch->GetPatchBox();
		int p = pPatch->GetPatchIndex();
		const DataArray1D<double> & dA = pPatch->GetANodes();
		const DataArray1D<double> & dB = pPatch->GetBNodes();
		// edges: 0=right,1=top,2=left,3=bottom (Direction enum order)
		for (int e = 0; e < 4; e++) {
			int ixPanel = pPatch->GetNeighborPanel((Direction)e);
			if (ixPanel == box.GetPanel()) continue;
			bool alongB = (e == 0) || (e == 2);
			int nAlong = alongB ? box.GetBTotalWidth() : box.GetATotalWidth();
			int fixed;
			if (e == 0) fixed = box.GetAInteriorEnd();
			else if (e == 1) fixed = box.GetBInteriorEnd();
			else if (e == 2) fixed = box.GetAInteriorBegin() - 1;
			else fixed = box.GetBInteriorBegin() - 1;
			std::vector<double> m(nAlong * 4);
			for (int s = 0; s < nAlong; s++) {
				int i = alongB ? fixed : s;
				int j = alongB ? s : fixed;
				double X = tan(dA[i]), Y = tan(dB[j]);
				double a0 = 1.0, b0 = 0.0, a1 = 0.0, b1 = 1.0;
				CubedSphereTrans::CoVecPanelTrans(ixPanel, box.GetPanel(), a0, b0, X, Y);
				CubedSphereTrans::CoVecPanelTrans(ixPanel, box.GetPanel(), a1, b1, X, Y);
				// out = M * in, column 0 = image of (1,0), column 1 = image of (0,1)
				m[4*s+0] = a0; m[4*s+1] = a1; m[4*s+2] = b0; m[4*s+3] = b1;
			}
			char nm[64]; snprintf(nm, 64, "halo_trans/p%d/e%d", p, e);
			w.f64(nm, D3(nAlong, 2, 2), &m[0]);
			snprintf(nm, 64, "halo_trans/p%d/e%d_srcpanel", p, e);
			w.iscalar(nm, ixPanel);
		}
	}
}


// the instance-0 state of every patch (node, redge, tracers) and PRECT, saved and restored around the calls
struct Snapshot { std::vector<std::vector<double> > a; };
static void copyArray(std::vector<double> & v, double * p, size_t n, bool save) {
	if (save) v.assign(p, p + n); else memcpy(p, &v[0], n * sizeof(double));
}
static void snap(GridGLL * pGrid, Snapshot & s, bool save) {
	if (save) s.a.clear();
	size_t q = 0;
	for (int n = 0; n < pGrid->GetActivePatchCount(); n++) {
		GridPatch * pPatch = pGrid->GetActivePatch(n);
		DataArray4D<double> * arr[3] = { &pPatch->GetDataState(0, DataLocation_Node), &pPatch->GetDataState(0, DataLocation_REdge), &pPatch->GetDataTracers(0) };
		for (int m = 0; m < 3; m++) {
			DataArray4D<double> & A = *arr[m];
			if (save) s.a.push_back(std::vector<double>());
			copyArray(s.a[q++], &(A[0][0][0][0]), A.GetSize(0) * A.GetSize(1) * A.GetSize(2) * A.GetSize(3), save);
		}
	}
}
static void resetPrect(GridGLL * pGrid) {
	for (int n = 0; n < pGrid->GetActivePatchCount(); n++) {
		DataArray3D<double> & U = pGrid->GetActivePatch(n)->GetUserData2D();
		for (size_t i = 0; i < U.GetSize(1); i++) for (size_t j = 0; j < U.GetSize(2); j++) U[0][i][j] = 0.0;
	}
}
static void dumpPrect(TmxdWriter & w, GridGLL * pGrid, const std::string & tag) {
	for (int n = 0; n < pGrid->GetActivePatchCount(); n++) {
		GridPatch * pPatch = pGrid->GetActivePatch(n);
		const DataArray3D<double> & U = pPatch->GetUserData2D();
		std::vector<double> v(U.GetSize(1) * U.GetSize(2));
		for (size_t i = 0; i < U.GetSize(1); i++) for (size_t j = 0; j < U.GetSize(2); j++) v[i * U.GetSize(2) + j] = U[0][i][j];
		char nm[32]; snprintf(nm, 32, "/p%d", pPatch->GetPatchIndex());
		w.f64("prect/" + tag + nm, D2(U.GetSize(1), U.GetSize(2)), &v[0]);
	}
}

int main(int argc, char ** argv) {
	TempestInitialize(&argc, &argv);
	std::string mode = "percall", tcase = "tc", out;
	int ne = 2, levels = 30, warm = 2, nsteps = 3, pbl = 1, prec = 1;
	double dt = 300.0, ztop = 30000.0, moisten = 0.0;
	for (int i = 1; i < argc; i++) {
		std::string a = argv[i];
		const char * v = (i + 1 < argc) ? argv[i+1] : "";
		if (a == "--mode") { mode = v; i++; }
		else if (a == "--case") { tcase = v; i++; }
		else if (a == "--out") { out = v; i++; }
		else if (a == "--ne") { ne = atoi(v); i++; }
		else if (a == "--levels") { levels = atoi(v); i++; }
		else if (a == "--warm") { warm = atoi(v); i++; }
		else if (a == "--steps") { nsteps = atoi(v); i++; }
		else if (a == "--pbl") { pbl = atoi(v); i++; }
		else if (a == "--prec") { prec = atoi(v); i++; }
		else if (a == "--dt") { dt = atof(v); i++; }
		else if (a == "--ztop") { ztop = atof(v); i++; }
		else if (a == "--moisten") { moisten = atof(v); i++; }
		else { fprintf(stderr, "unknown arg %s\n", a.c_str()); return 2; }
	}
	if (out == "" || (tcase != "tc" && tcase != "bw")) { fprintf(stderr, "need --out and --case tc|bw\n"); return 2; }
try {
	AnnounceSetVerbosityLevel(0);
	const bool fTC = (tcase == "tc");
	const int test = fTC ? 2 : 1;
	EquationSet eqn(EquationSet::PrimitiveNonhydrostaticEquations);
	eqn.InsertTracer("RhoQv", "RhoQv"); eqn.InsertTracer("RhoQc", "RhoQc"); eqn.InsertTracer("RhoQr", "RhoQr");
	if (!fTC) { eqn.InsertTracer("RhoQCl", "RhoQCl"); eqn.InsertTracer("RhoQCl2", "RhoQCl2"); }
	UserDataMeta metaUserData;
	metaUserData.InsertDataItem2D("PRECT");
	Model model(eqn, metaUserData);
	int isec = (int)dt;
	Time timeDeltaT(0, 0, 0, isec, 0, Time::CalendarNoLeap, Time::TypeDelta);
	model.SetDeltaT(timeDeltaT);
	model.SetEndTime(model.GetStartTime());      // Model::Go performs its initialisation only
	// TempestSetupCubedSphereModel defaults (src/atm/TempestInitialize.h): ARS343, np 4, hyperviscosity order 4 at 1e15, Lorenz
	model.SetTimestepScheme(new TimestepSchemeARS343(model));
	model.SetHorizontalDynamics(new HorizontalDynamicsFEM(model, 4, 4, 1.0e15, 1.0e15, 1.0e15, 0.0));
	model.SetVerticalDynamics(new VerticalDynamicsFEM(model, 4, 1, 0, false, true, false));
	GridCSGLL * pGrid = new GridCSGLL(model);
	pGrid->DefineParameters();
	pGrid->SetParameters(levels, 6, ne, 4, 4, 1, Grid::VerticalDiscretization_FiniteElement, Grid::VerticalStaggering_Lorenz);
	pGrid->InitializeDataLocal();
	model.SetGrid(pGrid, 6);
	if (fTC) model.SetTestCase(new TropicalCycloneTest(ztop, 1.0));
	else model.SetTestCase(new BaroclinicWaveUMJSTest(ztop, 1.0));
	model.Go();

	TmxdWriter w;
	w.open(out);
	w.iscalar("cfg/ne", ne);
	w.iscalar("cfg/np", 4);
	w.iscalar("cfg/levels", levels);
	w.iscalar("cfg/npatch", pGrid->GetActivePatchCount());
	w.iscalar("cfg/ninstances", model.GetComponentDataInstances());
	w.iscalar("cfg/ntracers", fTC ? 3 : 5);
	w.iscalar("cfg/test", test);
	w.scalar("cfg/ztop", pGrid->GetZtop());
	w.scalar("cfg/dt", dt);
	Time time = model.GetStartTime();
	TimestepScheme * pTS = model.GetTimestepScheme();
	DCMIPPhysics physWarm(model, timeDeltaT, test, 1, 1);      // the warm-up steps: the tropical cyclone's --bryanpbl --rjprecip
	DCMIPPhysics physStep(model, timeDeltaT, test, pbl, prec);
	physWarm.Initialize(time);
	physStep.Initialize(time);
	resetPrect(pGrid);
	int nstep = 0;
	if (mode == "percall") {
		dumpGeometry(w, model, pGrid);
		dumpHaloTransforms(w, pGrid);
		std::vector<std::string> tags;
		tags.push_back("stock"); tags.push_back("warm"); if (moisten > 0.0) tags.push_back("moist");
		for (size_t t = 0; t < tags.size(); t++) {
			if (tags[t] == "warm") {
				for (int s = 0; s < warm; s++) { pTS->Step(nstep++ == 0, false, time, dt); time += timeDeltaT; physWarm.Perform(time); }
			} else if (tags[t] == "moist") {
				// test INPUT of our own (as oracle/ref_dump.cpp --moisten): vapour scaled up, cloud and rain water in closed form,
				// the wind scaled by 0.5 .. 10, so that every branch of the subroutine acts on the coarse grid
				for (int n = 0; n < pGrid->GetActivePatchCount(); n++) {
					GridPatch * pPatch = pGrid->GetActivePatch(n);
					const PatchBox & box = pPatch->GetPatchBox();
					DataArray4D<double> & dT = pPatch->GetDataTracers(0);
					DataArray4D<double> & dN = pPatch->GetDataState(0, DataLocation_Node);
					const DataArray2D<double> & dLon = pPatch->GetLongitude();
					const DataArray2D<double> & dLat = pPatch->GetLatitude();
					const DataArray3D<double> & dZ = pPatch->GetZLevels();
					for (int i = box.GetAInteriorBegin(); i < box.GetAInteriorEnd(); i++)
					for (int j = box.GetBInteriorBegin(); j < box.GetBInteriorEnd(); j++)
					for (int k = 0; k < pGrid->GetRElements(); k++) {
						const double s1 = 0.5 * (1.0 + sin(3.0 * dLon[i][j]) * cos(2.0 * dLat[i][j]));
						dT[0][i][j][k] *= 1.0 + (moisten - 1.0) * s1;
						dT[1][i][j][k] = dN[4][i][j][k] * ((dZ[i][j][k] < 9000.0) ? 0.003 * s1 * s1 : 0.0);
						dT[2][i][j][k] = dN[4][i][j][k] * ((dZ[i][j][k] < 12000.0 && s1 > 0.3) ? 0.006 * (s1 - 0.3) : 0.0);
						dN[0][i][j][k] *= 0.5 + 9.5 * s1;
						dN[1][i][j][k] *= 0.5 + 9.5 * s1;
					}
				}
			}
			Snapshot s0;
			snap(pGrid, s0, true);
			dumpState(w, pGrid, tags[t], 0);
			for (int c = 0; c < 5; c++) {
				const int tc = (c == 4) ? 3 : test, pb = (c == 4) ? 0 : (c >> 1), pr = (c == 4) ? 0 : (c & 1);
				char nm[64]; snprintf(nm, 64, "%s_t%d_pbl%d_prec%d", tags[t].c_str(), tc, pb, pr);
				snap(pGrid, s0, false);
				resetPrect(pGrid);
				DCMIPPhysics phys(model, timeDeltaT, tc, pb, pr);
				phys.Initialize(time);
				phys.Perform(time);
				dumpState(w, pGrid, nm, 0);
				dumpPrect(w, pGrid, nm);
			}
			snap(pGrid, s0, false);
			resetPrect(pGrid);
		}
	} else if (mode == "steps") {
		for (int s = 0; s < warm; s++) { pTS->Step(nstep++ == 0, false, time, dt); time += timeDeltaT; physWarm.Perform(time); }
		dumpState(w, pGrid, "warm", 0);
		resetPrect(pGrid);
		for (int s = 1; s <= nsteps; s++) {
			pTS->Step(nstep++ == 0, false, time, dt); time += timeDeltaT; physStep.Perform(time);
			char nm[32]; snprintf(nm, 32, "step%d", s);
			dumpState(w, pGrid, nm, 0);
		}
		dumpPrect(w, pGrid, "steps");
	} else { fprintf(stderr, "bad --mode\n"); return 2; }
	w.close();
} catch (Exception & e) {
	fprintf(stderr, "%s\n", e.ToString().c_str());
	return 1;
}
	TempestDeinitialize();
	return 0;
}
