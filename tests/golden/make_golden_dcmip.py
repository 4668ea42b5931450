#!/usr/bin/env python3
"""Regenerate the DCMIP2016 column-physics fixtures from the REAL reference (only where /root/reference exists, after build()
has made oracle/_ref/libtempestref.a).  Nothing in build(), smoke(), bench.py or the tests calls this.

tests/native/dcmip_ref_dump.cpp is built in a temporary directory against the reference's own DCMIPPhysics.cpp,
TerminatorPhysics.cpp (g++ at oracle/Makefile's REFFLAGS) and Fortran halves (amdflang -O3 -fPIC), compiled where they lie.

  dcmip_tc_ne2_L6_p6.npz    TropicalCycloneTest (test 2, 3 tracers): geometry, then for two starting states -- the stock
                            state and the state after 2 ARS343 steps each followed by DCMIPPhysics::Perform(pbl 1, prec 1) --
                            the state after Perform for every (pbl, prec) in {0,1}^2 and for test 3; PRECT of every call;
                            branch counters
  dcmip_tc_moist_ne2_L6_p6.npz   the same for the third starting state, a moistened, wind-boosted copy of the warm one (test
                            input: every branch acts)
  dcmip_bw_ne2_L6_p6.npz, dcmip_bw_moist_ne2_L6_p6.npz   BaroclinicWaveUMJSTest (test 1, 5 tracers): the same per-call data
  dcmip_tc_steps_ne2_L6_p6.npz   the tropical cyclone after 3 more ARS343 steps, each followed by Perform, for
                            (pbl, prec) = (0, 0) and (1, 1), starting from the warm state of dcmip_tc_ne2_L6_p6.npz (the
                            warm-up steps use pbl 1, prec 1; the state is not stored twice)
Both cases run with ztop = 4.5 km in 6 levels on the ne2 grid of 6 patches (the smallest grid with a GLL node at the polar panel
centres).
States after a call are stored as the bitwise XOR with the state they started from (tests/dcmip_common.py: decode_after).

tests/dcmip_common.py: SLIM lists further shapes (tests/test_gpu_dcmip_levels.py; what each reaches: DESIGN.md section 2).  Each gets ONE slim file per
case, dcmip_<case>_slim_ne<ne>_L<L>_z<ztop>_dt<dt>_p6.npz, holding only what the physics reads and what the tests compare: cfg/,
phys/, per patch lat, a_nodes, b_nodes and the level and interface height columns, the MOIST starting state, its five calls as XOR
against it, PRECT of each call and the branch counters.  The metric geometry, the operators and the stock and warm states are left
out: the physics reads none of the metric, and the tests build the engine's grid object with golden_util.make_grid and upload
everything else from the file (tests/dcmip_common.py: slim_setup).

A file whose arrays have not changed is left as it is on disk (a .npz carries the time it was written: byte-identical fixtures
stay byte-identical).
"""
import os
import shutil
import subprocess
import sys
import tempfile
import glob
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import tmxd  # noqa: E402
import dcmip_common as dc  # noqa: E402
from make_golden import compact_states, flat_geometry, save  # noqa: E402

REF = "/root/reference"
CONDA = "/opt/conda"
F90 = "/opt/rocm/bin/amdflang"
REFFLAGS = ["-std=c++11", "-O2", "-fPIC", "-w", "-DTEMPEST_MPIOMP", "-DTEMPEST_LAPACK_FORTRAN_INTERFACE",
            "-I%s/src/base" % REF, "-I%s/src/atm" % REF, "-I%s/include" % CONDA, "-I%s/test/dcmip2016" % REF]
ENV = dict(os.environ, MKL_THREADING_LAYER="SEQUENTIAL")
# ztop 4.5 km in 6 levels of 750 m: interface 1 lies inside the Bryan boundary layer (0 < zi < zpbltop, a non-zero diffusivity),
# the others above it, and presi crosses pbltop a few interfaces up, so both sides of both boundary-layer tests act
NE, L, DT, ZTOP = 2, 6, 300.0, 4500.0
# the slim fixtures' shapes, id -> (ne, L, ztop, dt, cases), and their file names: tests/dcmip_common.py (SLIM, slim_name), which the tests read too
COMBOS = ["t%d_pbl%d_prec%d" % (2, pb, pr) for pb in (0, 1) for pr in (0, 1)]


def build(tmp):
    dc = os.path.join(REF, "test", "dcmip2016")
    objs = []
    for f in ("dcmip_physics_z_v1", "kessler", "tropical_cyclone_test", "baroclinic_wave_test", "Terminator"):
        o = os.path.join(tmp, "f_%s.o" % f)
        subprocess.check_call([F90, "-O3", "-fPIC", "-c", os.path.join(dc, "interface", f + ".f90"), "-o", o], cwd=tmp)
        objs.append(o)
    for src in (os.path.join(dc, "DCMIPPhysics.cpp"), os.path.join(dc, "TerminatorPhysics.cpp"),
                os.path.join(ROOT, "tests", "native", "dcmip_ref_dump.cpp")):
        o = os.path.join(tmp, os.path.basename(src) + ".o")
        subprocess.check_call(["g++"] + REFFLAGS + ["-c", src, "-o", o])
        objs.append(o)
    rt = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/x86_64-unknown-linux-gnu/libflang_rt.runtime.a"))[0]
    exe = os.path.join(tmp, "dcmip_ref_dump")
    subprocess.check_call(["g++", "-o", exe] + objs + [os.path.join(ROOT, "oracle", "_ref", "libtempestref.a"), rt,
                          CONDA + "/lib/libmpicxx.so", CONDA + "/lib/libmpi.so", CONDA + "/lib/libmkl_rt.so",
                          "-Wl,-rpath,/usr/lib/x86_64-linux-gnu", "-Wl,-rpath," + CONDA + "/lib", "-ldl"])
    return exe


def run(exe, tmp, args):
    out = os.path.join(tmp, "dump.tmxd")
    subprocess.run([exe] + args + ["--out", out], env=ENV, check=True, stdout=subprocess.DEVNULL)
    return tmxd.read(out)


def branch_counts(d, tag, test):
    """How many columns (interfaces) of a starting state meet each branch of DCMIP2016_PHYSICS, from the state before the
    call (an estimate in numpy arithmetic, for the record) and the reference's precipitation of the calls."""
    Rd, cp, p0 = 287.0, 1004.5, 100000.0
    gam = cp / (cp - Rd)
    c = {}
    n_rj = n_w_lo = n_w_hi = n_pre_hi = n_pre_lo = n_zi_lo = n_zi_hi = n_zi_in = 0
    for p in range(6):
        node = d["state/%s/p%d/node" % (tag, p)][:, 1:-1, 1:-1]
        tr = d["state/%s/p%d/tracers" % (tag, p)][:, 1:-1, 1:-1]
        rho, rt = node[4], node[2]
        pr = p0 * (Rd * rt / p0) ** gam
        qv = np.maximum(tr[0] / rho, 0.0)
        rhod = rho - tr[0] - tr[1] - tr[2]
        rhom = rhod * (1.0 + qv)
        t = pr / (rhom * Rd * (1.0 + (461.5 / 287.0 - 1.0) * qv))
        qsv = qv * rhod / rhom
        qsat = (287.0 / 461.5) * 610.78 / pr * np.exp(-(2.5e6 / 461.5) * (1.0 / t - 1.0 / 273.16))
        n_rj += int(np.sum(np.any(qsv > qsat, axis=-1)))
        # lowest-level wind speed from (U, V) through the contravariant 2-D metric (GetContraMetric2DA/B)
        ca, cb = d["p%d/contra_metric_2d_a" % p][1:-1, 1:-1], d["p%d/contra_metric_2d_b" % p][1:-1, 1:-1]
        u, v = node[0, ..., 0], node[1, ..., 0]
        w2 = u * (ca[..., 0] * u + ca[..., 1] * v) + v * (cb[..., 0] * u + cb[..., 1] * v)
        wind = np.sqrt(np.maximum(w2, 0.0)) * float(d["phys/earth_radius"][0])     # (the 2-D metric carries 1 / a^2)
        n_w_lo += int(np.sum(wind < 20.0)); n_w_hi += int(np.sum(wind >= 20.0))
        presi = 0.5 * (pr[..., :-1] + pr[..., 1:])
        n_pre_hi += int(np.sum(presi >= 85000.0)); n_pre_lo += int(np.sum(presi < 85000.0))
        zi = d["p%d/z_interfaces" % p][1:-1, 1:-1, 1:-1]
        n_zi_lo += int(np.sum(zi <= 1000.0)); n_zi_hi += int(np.sum(zi > 1000.0)); n_zi_in += int(np.sum((zi > 0.0) & (zi < 1000.0)))
    c["rj_supersaturated_columns"] = n_rj
    c["wind_below_20_columns"] = n_w_lo
    c["wind_above_20_columns"] = n_w_hi
    c["presi_ge_pbltop_interfaces"] = n_pre_hi
    c["presi_lt_pbltop_interfaces"] = n_pre_lo
    c["zi_le_zpbltop_interfaces"] = n_zi_lo
    c["zi_gt_zpbltop_interfaces"] = n_zi_hi
    c["zi_inside_bryan_pbl_interfaces"] = n_zi_in      # 0 < zi < zpbltop: a non-zero Bryan diffusivity
    for pr_ in (0, 1):
        k = "prect/%s_t%d_pbl0_prec%d/" % (tag, test, pr_)
        c["precipitating_columns_prec%d" % pr_] = int(sum(np.sum(d[k + "p%d" % p][1:-1, 1:-1] > 0.0) for p in range(6)))
    return c


def save_if_changed(name, rec):
    """make_golden.save, unless the file on disk already holds exactly these arrays (names, types, shapes, bits)."""
    path = os.path.join(HERE, name)
    if os.path.exists(path):
        with np.load(path) as z:
            old = {k.replace("__", "/"): z[k] for k in z.files}
        if set(old) == set(rec) and all(old[k].dtype == np.asarray(rec[k]).dtype and old[k].shape == np.asarray(rec[k]).shape
                                        and old[k].tobytes() == np.ascontiguousarray(rec[k]).tobytes() for k in rec):
            print(name, "unchanged, %.2f MB" % (os.path.getsize(path) / 1e6))
            return
    save(name, rec)


PART_LIMIT = 1 << 20      # no committed file is larger than 1 MiB


def save_slim(name, rec):
    """One slim fixture, cut where it is larger than PART_LIMIT: <name> holds everything but the calls' states, and as many
    calls' XOR arrays as fit; the following calls go to <name less .npz>.part1.npz, ... (tests/dcmip_common.py: load_slim joins
    them).  Parts left over from an earlier, longer cut are removed."""
    calls = sorted({k.split("/")[1] for k in rec if k.startswith("xor/")})
    groups = [{k: v for k, v in rec.items() if not k.startswith("xor/")}] + [{k: v for k, v in rec.items() if k.startswith("xor/%s/" % c)} for c in calls]
    probe = os.path.join(tempfile.gettempdir(), "dcmip_probe_%d.npz" % os.getpid())

    def size(r):
        np.savez_compressed(probe, **{k.replace("/", "__"): v for k, v in r.items()})
        n = os.path.getsize(probe); os.remove(probe)
        return n
    parts, cur = [], groups[0]
    for g in groups[1:]:
        both = dict(cur); both.update(g)
        if size(both) <= PART_LIMIT:
            cur = both
        else:
            parts.append(cur); cur = g
    parts.append(cur)
    stem = name[:-len(".npz")]
    names = [name] + ["%s.part%d.npz" % (stem, i) for i in range(1, len(parts))]
    for stale in glob.glob(os.path.join(HERE, stem + ".part*.npz")):
        if os.path.basename(stale) not in names:
            os.remove(stale)
    for n, r in zip(names, parts):
        save_if_changed(n, r)
        assert os.path.getsize(os.path.join(HERE, n)) <= PART_LIMIT, n


def percall(exe, tmp, case, name, ne=NE, nlev=L, ztop=ZTOP, dt=DT, slim=False):
    test = 2 if case == "tc" else 1
    d = run(exe, tmp, ["--case", case, "--mode", "percall", "--ne", str(ne), "--levels", str(nlev), "--dt", str(dt),
                       "--ztop", str(ztop), "--warm", "2", "--pbl", "1", "--prec", "1", "--moisten", "1.5"])
    rec = {k: v for k, v in d.items() if k.startswith(("cfg/", "phys/") if slim else ("cfg/", "phys/", "grid/"))}
    if not slim:
        rec.update(flat_geometry(d))
    for p in range(6):
        for nm in ("a_nodes", "b_nodes", "lat"):
            rec["p%d/%s" % (p, nm)] = d["p%d/%s" % (p, nm)]
        # no topography: one column of level and interface heights serves every node
        for nm in ("z_levels", "z_interfaces"):
            z = d["p%d/%s" % (p, nm)]
            assert np.array_equal(z, np.broadcast_to(z[1, 1], z.shape)), nm
            rec["p%d/dcmip_%s" % (p, nm)] = z[1, 1].copy()
    cs = compact_states(d, 6)
    starts = ("stock", "warm", "moist")
    for k, v in cs.items():
        tag = k.split("/")[1]
        if tag in starts:
            rec[k] = v
            continue
        # the state after a call, stored as the bitwise XOR with the state it started from (decode_after in the tests):
        # W and the tracers beyond the third are not touched by Perform (checked here and left out)
        base = cs[k.replace(tag, tag.split("_")[0], 1)]
        if k.endswith("/redge"):
            assert np.array_equal(v, base), k
            continue
        if k.endswith("/tracers"):
            assert np.array_equal(v[3:], base[3:]), k
            v, base = v[:3], base[:3]
        rec[k.replace("state/", "xor/", 1)] = np.bitwise_xor(v.view(np.uint64), base.view(np.uint64))
    for k, v in d.items():
        if k.startswith("prect/"):
            rec[k] = v
    print(name)
    for tag in ("moist",) if slim else ("stock", "warm", "moist"):
        cnt = branch_counts(d, tag, test)
        for k, v in cnt.items():
            rec["branches/%s/%s" % (tag, k)] = np.array([v], dtype=np.int64)
        print("  %-6s" % tag, " ".join("%s=%d" % kv for kv in cnt.items()))
    # the moistened state's calls in a file of their own (tests/dcmip_common.py: load_case joins the two)
    moist = {k: v for k, v in rec.items() if k.split("/")[1].startswith("moist")}
    if slim:
        # one file: what the physics reads (cfg, phys, lat, node angles, height columns) and the moist state's calls
        keep = {k: v for k, v in rec.items() if k in moist or k.startswith(("cfg/", "phys/")) or k.split("/")[0][0] == "p" and k[1].isdigit()}
        assert all(np.all(np.isfinite(v)) for k, v in keep.items() if v.dtype == np.float64), name
        save_slim(name, keep)
        return cs
    save_if_changed(name, {k: v for k, v in rec.items() if k not in moist})
    save_if_changed(name.replace("_ne", "_moist_ne", 1), moist)
    return cs


def steps(exe, tmp, name, warm):
    rec = {}
    for pb, pr in ((0, 0), (1, 1)):
        d = run(exe, tmp, ["--case", "tc", "--mode", "steps", "--ne", str(NE), "--levels", str(L), "--dt", str(DT),
                           "--ztop", str(ZTOP), "--warm", "2", "--steps", "3", "--pbl", str(pb), "--prec", str(pr)])
        cs = compact_states(d, 6)
        for k, v in cs.items():
            tag = k.split("/")[1]
            if tag == "warm":
                # both runs start from the per-call fixture's warm state (the same two steps): the tests read it from there
                assert np.array_equal(warm[k], v), k
            elif tag == "step3":
                rec[k.replace("state/step3/", "xor/pbl%d_prec%d_step3/" % (pb, pr), 1)] = np.bitwise_xor(
                    v.view(np.uint64), cs[k.replace("step3", "warm", 1)].view(np.uint64))
        for p in range(6):
            rec["prect/pbl%d_prec%d_steps/p%d" % (pb, pr, p)] = d["prect/steps/p%d" % p]
        rec["cfg/dt"] = d["cfg/dt"]
    save_if_changed(name, rec)


def main():
    if not os.path.isdir(os.path.join(REF, "test", "dcmip2016")):
        sys.exit("needs the reference sources")
    tmp = tempfile.mkdtemp()
    try:
        exe = build(tmp)
        only = sys.argv[1:]      # ids of dcmip_common.SLIM: those slim files alone; none: every file
        if not only:
            tc = percall(exe, tmp, "tc", "dcmip_tc_ne%d_L%d_p6.npz" % (NE, L))
            percall(exe, tmp, "bw", "dcmip_bw_ne%d_L%d_p6.npz" % (NE, L))
            steps(exe, tmp, "dcmip_tc_steps_ne%d_L%d_p6.npz" % (NE, L), tc)
        for sid, (ne, nlev, ztop, dt, cases) in dc.SLIM.items():
            for case in cases:
                if not only or sid in only:
                    percall(exe, tmp, case, dc.slim_name(sid, case) + ".npz", ne, nlev, float(ztop), float(dt), slim=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
