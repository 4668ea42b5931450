#!/usr/bin/env python3
"""Time tmx_physics_dcmip2016 per (pbl_type, prec_type) next to tmx_physics_kessler on the same moist state: ne30 np4, 24 patches,
L30 and L60 (ztop 30 km), three tracers, one GPU.  The state is the synthesiser's baroclinic wave with prescribed vapour / cloud /
rain profiles (the tropical cyclone's initial state needs the reference's Fortran initialiser); every call restarts from it, so
every call does the same work.  Prints one line per shape and variant: microseconds per call (median of K calls, each synchronised)
and the minimal HBM traffic of the kernel.  Usage: tools/dcmip_timing.py [ne] [K]  (run on the GPU box; rocprofv3 --kernel-trace
--stats around it gives the kernel times without the host)."""
import os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import golden_util as gu
from tempestmodel_amd.engine import Engine

ne = int(sys.argv[1]) if len(sys.argv) > 1 else 30
K = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dt = 300.0


def timed(e, states, tracers, fn):
    ts = []
    for i in range(K + 3):
        e.upload_state(0, states); e.upload_tracers(0, tracers); e.sync()
        t0 = time.perf_counter()
        fn(); e.sync()
        if i >= 3:
            ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts))


for L in (30, 60):
    g, states = gu.make_grid(ne, L, 24, ztop=30000.0, ntracers=3)
    tracers = []
    for P, (n, _) in zip(g.patches, states):
        z = P.geom["z_levels"]; rho = n[4]
        qv = 0.018 * np.exp(-z / 2500.0); qc = 2.0e-4 * np.exp(-((z - 3000.0) / 1500.0) ** 2); qr = 1.0e-4 * np.exp(-((z - 2000.0) / 1500.0) ** 2)
        tracers.append(np.stack([rho * qv, rho * qc, rho * qr]))
    for opt in (0, 1):
        e = Engine(g, options={"dcmip_lds": opt})
        e.set_level_heights(); e.set_dcmip_inputs()
        if opt == 0:
            print("ne%d L%d kessler: %.1f us per call" % (ne, L, timed(e, states, tracers, lambda: e.kessler(0, dt))))
        ncol = 6 * ne * ne * 16
        # minimal traffic: read U, V, rho*theta, rho, 3 tracers, z levels and interfaces, 10 coefficients; write U, V, rho*theta, rho, 3 tracers
        byt = 8.0 * ncol * (L * (7 + 1 + 7) + (L + 1) + 11)
        for pbl in (0, 1):
            for prec in (0, 1):
                us = timed(e, states, tracers, lambda: e.dcmip2016(0, dt, 2, pbl, prec))
                print("ne%d L%d dcmip pbl %d prec %d (%s): %.1f us per call, minimal HBM traffic %.1f MB (%.2f TB/s at that time)"
                      % (ne, L, pbl, prec, "Thomas arrays in LDS" if opt and L * 6 * 512 <= 160 * 1024 else "Thomas arrays in HBM", us, byt / 1e6, byt / us / 1e6))
        e.close()
