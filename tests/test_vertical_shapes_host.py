"""The kernel shape every launcher of the vertical family picks from the level count, swept on the CPU from 3 to 330 levels through
tmx_debug_vertical_shape (the host functions the launchers themselves call: tmx_internal.h), against a restatement of the launchers' LDS
formulas written out here and in the two GPU files that own the kernels (test_gpu_column_solve_levels.py, test_gpu_tracer_column_shapes.py).
No shape may ask for more than the 160 KB of LDS a CU has; "does not fit" starts exactly where the restated bytes say and never ends again;
the refusal names the kernel and the largest level count it serves.  And the inputs of the GPU tests above 60 levels are qualified on the C
oracle: every call and step returns 0, stays finite and changes state and tracers -- a GPU comparison with a vacuous expectation fails here.

Thresholds (first level count of the new shape), all asserted below:

    tmxk_vi_fused        two pairs per workgroup: ring rows 3 -> 2 at 37, -> 3 at 83, -> 2 at 223 (three rows need 440 L + 66 000 bytes), one pair per
                         workgroup from 269 (two rows: 440 L + 45 520); one pair: 3 -> 2 at 110, -> 3 at 133, -> 2 at 301, nothing fits from 325
                         (428 L + 25 012); two producers (428 L + 45 492) -> one from 277; lane-group kernel -> pair kernel from 160 (its ring of 480
                         doubles per column receives the 3 (L + 1) solution entries)
    launch_vt_solve      row lanes <16, 3> -> <32, 4> at 49 -> <1, 3> at 142; one row lane: 64 -> 32 columns at 36, -> 16 at 71, -> 8 at 142; refusal from 285
    the three walks      terms kernel (416 L + 4 504 bytes against 64 KB) level-parallel from 147, U,V penalty and tracers (416 L + 408) from 157
    vt_column            64 -> 32 columns at 80, refusal from 160

No level count puts a working set exactly ON its limit (no restated byte count equals 160 KB, half of it or 64 KB for an integer L: asserted), so
`<=` and `<` in a fit test choose alike at every level count; what the sweep pins is the last level count on either side of each limit."""
import ctypes as C
import numpy as np
import pytest
import golden_util as gu
import test_gpu_column_solve_levels as csl
import test_gpu_tracer_column_shapes as tcs
from test_gpu_column_solve_levels import _pair_lds, _auto_ring_depth, _group_serves, CU_LDS
from test_gpu_tracer_column_shapes import _expected_vt, _expected_walks, _segments

LEVELS = range(3, 331)


def _fn():
    from tempestmodel_amd import engine as eng
    fn = eng.load_library().tmx_debug_vertical_shape
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_longlong)]
    return fn


def _shape(launcher, L, *args, engine=None):
    a = (C.c_int * max(1, len(args)))(*args)
    out = (C.c_longlong * 4)()
    r = _fn()(engine, launcher, L, a, len(args), out)
    return r, list(out)


def _predict_vi(L, nunique, closed, group, pair_wg, producers, ring_depth, cpw=64, group_max=6400):
    """(kernel, pairs, producers, ring rows, bytes) tmxk_vi_fused must choose, or None where nothing fits: the present choice wherever it fits,
    else a smaller shape of the pair kernel -- one assembly wavefront, two ring rows, one pair per workgroup."""
    if _group_serves(L) and (group == 1 or (group < 0 and nunique <= group_max)):
        return (2, 0, 0, 0, 0)
    ngrp = -(-nunique // cpw)
    pairs = pair_wg if pair_wg > 0 else (1 if ngrp <= 256 else 2)
    two = bool(closed) and pairs == 1 and cpw == 64 and (producers == 2 or (producers == 0 and ngrp * 3 <= 1024))
    while True:
        if two:
            ring = 4
        else:
            ring = ring_depth if ring_depth in (2, 3) else _auto_ring_depth(L, pairs)
            if ring == 3 and _pair_lds(L, pairs, 3) > CU_LDS:
                ring = 2
        if _pair_lds(L, pairs, ring) <= CU_LDS:
            return (1, pairs, 2 if two else 1, ring, _pair_lds(L, pairs, ring))
        if two:
            two = False
        elif pairs > 1:
            pairs = 1
        else:
            return None


# (name, unique columns, closed-form metric, vi_group, vi_pair_workgroup, vi_producers, vi_ring_depth); 488 unique columns = 8 column groups (the
# GPU tests' grid), 100 000 = 1 563 groups (a production-sized rank: two pairs per workgroup on its own)
VI_CONFIGS = [(n, nu, cl, gr, pw, pr, rd) for nu, tag in ((488, "small"), (100000, "large")) for cl in (1, 0) for gr in (0, 1, -1)
              for pw in (0, 1, 2) for pr in (0, 1, 2) for rd in (0, 2, 3) for n in ["%s_cl%d_g%d_pw%d_pr%d_rd%d" % (tag, cl, gr, pw, pr, rd)]]


def test_column_solve_shapes_swept_over_levels():
    """Every combination of one / two / automatic pairs, one / two / automatic producers, closed and stored metric, each forced ring depth, the
    lane-group kernel on, off and automatic, on a small and on a production-sized column count."""
    ranges = {}
    for name, nu, cl, gr, pw, pr, rd in VI_CONFIGS:
        refused_from = None
        for L in LEVELS:
            r, out = _shape(0, L, nu, 64, cl, 1 << 30, gr, 6400, pw, pr, rd)
            want = _predict_vi(L, nu, cl, gr, pw, pr, rd)
            assert out[2] <= CU_LDS or r == 1, (name, L, out)      # no shape that is launched asks for more than a CU has
            if want is None:
                refused_from = refused_from or L
                assert r == 1 and out[0] == -1 and out[3] == refused_from - 1, (name, L, r, out)
            else:
                assert refused_from is None, (name, L)      # "does not fit" never ends again
                k, p, q, ring, b = want
                assert r == 0 and out[0] == k and out[1] == (p | q << 4 | ring << 8 if k == 1 else 0) and out[2] == b and out[3] == 0, (name, L, out, want)
                ranges.setdefault(name, {}).setdefault((k, p, q, ring), []).append(L)
        assert refused_from == 325, (name, refused_from)      # one pair, two rows: 428 L + 25 012 bytes
    span = lambda name: {k: (v[0], v[-1]) if v == list(range(v[0], v[-1] + 1)) else v for k, v in ranges[name].items()}
    # two pairs per workgroup, one assembly wavefront, automatic ring depth (what every grid above 256 column groups runs)
    assert span("large_cl1_g0_pw0_pr0_rd0") == {(1, 2, 1, 3): list(range(3, 37)) + list(range(83, 223)), (1, 2, 1, 2): list(range(37, 83)) + list(range(223, 269)),
                                                (1, 1, 1, 3): (269, 300), (1, 1, 1, 2): (301, 324)}
    assert ranges["large_cl1_g0_pw2_pr0_rd0"] == ranges["large_cl1_g0_pw0_pr0_rd0"] == ranges["small_cl0_g0_pw2_pr2_rd0"]
    # ... with the ring depth forced: 3 holds up to 222 levels, 2 up to 268
    assert span("large_cl1_g0_pw2_pr0_rd3") == {(1, 2, 1, 3): (3, 222), (1, 2, 1, 2): (223, 268), (1, 1, 1, 3): (269, 300), (1, 1, 1, 2): (301, 324)}
    assert span("large_cl1_g0_pw2_pr0_rd2") == {(1, 2, 1, 2): (3, 268), (1, 1, 1, 2): (269, 324)}
    # one pair per workgroup, one producer
    assert span("small_cl1_g0_pw1_pr1_rd0") == {(1, 1, 1, 3): list(range(3, 110)) + list(range(133, 301)), (1, 1, 1, 2): list(range(110, 133)) + list(range(301, 325))}
    # two producers (forced, or the default of a small grid with the lane-group kernel off): 428 L + 45 492 bytes up to 276 levels, then one
    for name in ("small_cl1_g0_pw1_pr2_rd0", "small_cl1_g0_pw0_pr0_rd0", "small_cl1_g0_pw0_pr2_rd3"):
        assert span(name) == {(1, 1, 2, 4): (3, 276), (1, 1, 1, 3): (277, 300), (1, 1, 1, 2): (301, 324)}, name
    # ... which need the closed-form metric
    assert ranges["small_cl0_g0_pw1_pr2_rd0"] == ranges["small_cl1_g0_pw1_pr1_rd0"]
    # the lane-group kernel (forced, or the default of a small grid) up to 159 levels, then the pair kernel in the shape the other options give
    assert span("small_cl1_g1_pw0_pr0_rd0") == span("small_cl1_g-1_pw0_pr0_rd0") == {(2, 0, 0, 0): (3, 159), (1, 1, 2, 4): (160, 276), (1, 1, 1, 3): (277, 300), (1, 1, 1, 2): (301, 324)}
    assert ranges["large_cl1_g-1_pw0_pr0_rd0"] == ranges["large_cl1_g0_pw0_pr0_rd0"]      # above vi_group_max columns: never
    # the byte formulas of the table, and: no level count puts a shape exactly on a limit
    for L in LEVELS:
        assert (_pair_lds(L, 2, 3), _pair_lds(L, 2, 2), _pair_lds(L, 1, 3), _pair_lds(L, 1, 2), _pair_lds(L, 1, 4)) == (
            440 * L + 66000, 440 * L + 45520, 428 * L + 35252, 428 * L + 25012, 428 * L + 45492)
        assert all(_pair_lds(L, p, d) not in (CU_LDS, CU_LDS // 2) for p in (1, 2) for d in (2, 3, 4))
    # a stream the lane-group kernel's 16 doubles per row and column do not fit (122 workgroups x 64 > 10 x 512): the pair kernel, as before
    assert _shape(0, 30, 488, 64, 1, 512, 1, 6400, 0, 0, 0)[1][0] == 1 and _shape(0, 30, 488, 64, 1, 781, 1, 6400, 0, 0, 0)[1][0] == 2


def test_tracer_column_shapes_swept_over_levels():
    """launch_vt_solve on the unique columns ("vt_lanes" = 16) and on every stored column (64), "vt_rows" 1 and 0: (9L + 3) doubles per column."""
    lds = lambda L, lw: (9 * L + 3) * lw * 8
    for all_columns in (0, 1):
        for rows in (1, 0):
            seen = {}
            for L in LEVELS:
                r, out = _shape(1, L, all_columns, rows, 0, -1, 16)
                if lds(L, 8) > CU_LDS:
                    assert L >= 285 and r == 1 and out[0] == 0 and out[3] == 284, (all_columns, rows, L, out)
                    continue
                want = _expected_vt(L, rows, bool(all_columns))
                assert r == 0 and out[0] | out[1] << 8 | all_columns << 16 == want and out[2] == lds(L, 1 << out[1]) <= CU_LDS and out[3] == 0, (all_columns, rows, L, out, want)
                seen.setdefault((out[0], out[1]), []).append(L)
            spans = {k: (v[0], v[-1]) for k, v in seen.items() if v == list(range(v[0], v[-1] + 1))}
            assert len(spans) == len(seen), seen
            if rows:
                assert spans == {(16, 3): (3, 48), (32, 4): (49, 141), (1, 3): (142, 284)}, (all_columns, spans)
            elif all_columns:
                assert spans == {(1, 6): (3, 35), (1, 5): (36, 70), (1, 4): (71, 141), (1, 3): (142, 284)}, spans
            else:
                assert spans == {(1, 4): (3, 141), (1, 3): (142, 284)}, spans
    assert all(lds(L, lw) != CU_LDS for L in LEVELS for lw in (8, 16, 32, 64))
    # the options that force a shape keep it where it fits: 8 row lanes x 16 columns at 141 levels, and the one-lane form takes over at 142 all the same
    assert _shape(1, 141, 0, 1, 8, 0, 16)[1][:2] == [8, 4] and _shape(1, 142, 0, 1, 8, 0, 16)[1][:2] == [1, 3]


def test_explicit_mode_kernels_swept_over_levels():
    """The three walks (automatic segment count on the GPU tests' 14 tiles and on 1 350, forced -1, -2, -64, and 0 = level-parallel) and the
    one-lane-per-column tracer kernel of "vt_column"."""
    walk = lambda L, extra: (10 * (L + 1) * 5 + 2 * L + 1 + extra) * 8
    names = ("vx_walk", "vt_explicit_walk", "vite_walk")
    for ntiles in (tcs.NTILES, 1350):
        for w in (-1000, -1, -2, -64, 0):
            first_zero = [None] * 3
            for L in LEVELS:
                got = [_shape(2 + i, L, w, ntiles) for i in range(3)]
                assert all(r == 0 for r, _ in got)
                if ntiles == tcs.NTILES:
                    want = _expected_walks(L, {n: w for n in names})
                    assert [o[0] for _, o in got] == [(want >> s) & 0xfff for s in (0, 12, 24)], (w, L, got)
                for i, (_, o) in enumerate(got):
                    extra, rows, target = (512, L + 1, 2048) if i == 2 else (0, L, 4096 if i == 0 else 2048)
                    if w < 0 and walk(L, extra) <= 64 * 1024:
                        assert first_zero[i] is None, (w, L, i)      # the level-parallel form, once taken, stays
                        assert o[0] == _segments(w, ntiles, rows, target) >= 1 and o[2] == walk(L, extra), (w, L, i, o)
                    else:
                        first_zero[i] = first_zero[i] or L
                        assert o[0] == 0 and o[2] == 0, (w, L, i, o)      # no dynamic LDS at all
            assert first_zero == ([3, 3, 3] if w == 0 else [157, 157, 147]), (w, first_zero)
    assert [walk(L, 0) for L in (117, 118, 156, 157)] == [416 * L + 408 for L in (117, 118, 156, 157)] and walk(117, 0) <= 48 * 1024 < walk(118, 0)
    assert walk(146, 512) == 416 * 146 + 4504 <= 64 * 1024 < walk(147, 512) and walk(156, 0) <= 64 * 1024 < walk(157, 0)
    assert all(walk(L, x) != 64 * 1024 for L in LEVELS for x in (0, 512))
    # StepImplicitTermsExplicitly with the U,V update fused in (experiments flavour) has no walk
    assert _shape(4, 30, -1000, 14, 1)[1][0] == 0 and _shape(4, 30, -1000, 14, 0)[1][0] > 0
    col = lambda L, lw: (4 * L + 2) * lw * 8
    for L in LEVELS:
        r, out = _shape(5, L)
        if L <= 79:
            assert (r, out) == (0, [64, 0, col(L, 64), 0]) and col(L, 64) <= CU_LDS, (L, out)
        elif L <= 159:
            assert (r, out) == (0, [32, 0, col(L, 32), 0]) and col(L, 64) > CU_LDS >= col(L, 32), (L, out)
        else:
            assert (r, out[0], out[3]) == (1, 0, 159) and col(L, 32) > CU_LDS, (L, out)
    assert all(col(L, lw) != CU_LDS for L in LEVELS for lw in (32, 64))


def test_refusals_name_the_kernel_and_its_limit():
    """Plan-only engines (device = -2) at refused level counts: the debug call answers what the ABI call would (TMX_ERR_UNSUPPORTED, the
    message with the kernel and the largest level count it serves), and reports that limit."""
    from tempestmodel_amd.engine import Engine
    cases = [(285, 1, {}, {}, 1, (0,), "k_vi_tracers_rows", 284), (285, 1, {}, {}, 1, (1,), "k_vi_tracers_rows", 284),
             (160, 1, {"vt_column": 1}, dict(fully_explicit=True), 5, (), "k_v_tracers_explicit_column", 159),
             (325, 0, {"vi_group": 0}, {}, 0, (), "k_vi_pair", 324)]
    for L, nt, options, mode, launcher, args, kernel, limit in cases:
        g, _ = gu.make_grid(2, L, 6, ntracers=nt)
        e = Engine(g, device=-2, options=options, **mode)
        try:
            r, out = _shape(launcher, 0, *args, engine=e.h)
            msg = e.lib.tmx_last_error().decode()
            print(L, launcher, r, out, msg)
            assert r == -2 and out[0] == -1 and out[3] == limit, (L, launcher, r, out)
            assert kernel in msg and "%d levels" % L in msg and "up to %d levels" % limit in msg, msg
        finally:
            e.close()
        # one level count less: fits, with the engine's own numbers
        g, _ = gu.make_grid(2, limit, 6, ntracers=nt)
        e = Engine(g, device=-2, options=options, **mode)
        try:
            r, out = _shape(launcher, 0, *args, engine=e.h)
            assert r == 0 and out[2] <= CU_LDS, (limit, launcher, r, out)
            if launcher == 0:
                assert (out[0], out[1]) == (1, 1 | 1 << 4 | 2 << 8), out      # a few column groups: one pair, one producer, two rows
        finally:
            e.close()
    assert _shape(9, 30)[0] == -1 and _shape(0, 30, 0)[0] == -1      # unknown launcher, no columns


# ---- the inputs of the GPU tests above 60 levels, qualified on the oracle -------------------------------------------------------------

def _all_finite(states, tracers=None):
    return all(np.isfinite(n).all() and np.isfinite(e).all() for n, e in states) and (tracers is None or all(np.isfinite(t).all() for t in tracers))


@pytest.mark.parametrize("L,ntr", csl.NEW_LEVELS, ids=["L%d" % L for L, _ in csl.NEW_LEVELS])
def test_column_solve_inputs_above_60_levels(L, ntr):
    """test_gpu_column_solve_levels.py's grid, smooth and rough state at the new level counts: V.StepImplicit per call, two ARS343 steps and a
    Strang step return 0 under both roundings of the band LU, stay finite (asserted in _oracle_expectations) and change state and tracers; the
    scrub step (dt = 37 from the initial state) returns 0 and ends elsewhere than the compared steps.  Whether the rough state's pivots diverge
    between the lanes of a wavefront is a property of the device's column-to-lane map that the oracle does not expose: it stays asserted on the
    device, through the pair kernel's own statistics, at every level count."""
    from oracle_lib import Oracle
    g, g0, states, tr0, smooth, tr, rough = csl._inputs(L, ntr)
    assert _all_finite(smooth, tr) and _all_finite(rough)
    for fma in sorted({int(o.get("lu_fma", 1)) for _, o in csl._variants(L)} | {1}):
        want = csl._oracle_expectations(g, smooth, rough, tr, fma)
        for key, start in (("rough", rough), ("smooth", smooth), ("steps", smooth)):
            assert 0.0 < max(gu.prognostic_errors(want[key][0], start)) < float("inf"), (L, fma, key)
            if ntr:
                assert 0.0 < max(gu.tracer_errors(want[key][1], tr)) < float("inf"), (L, fma, key)
    o = Oracle(g); o.set_state(0, states)
    if ntr:
        o.set_tracers(0, tr0)
    assert o.step_ars343(37.0) == 0
    assert _all_finite(o.get_state(0)) and 0.0 < max(gu.prognostic_errors(o.get_state(0), want["steps"][0])) < float("inf")
    # every variant run at this level count is one the sweep above says fits
    for name, options in csl._variants(L):
        assert _predict_vi(L, 488, "metric_stored" not in options, options.get("vi_group", -1), options.get("vi_pair_workgroup", 0), options.get("vi_producers", 0),
                           options.get("vi_ring_depth", 0)) is not None, (L, name)


@pytest.mark.parametrize("L,nt", tcs.NEW_SHAPES_IMPLICIT + [tcs.REFUSED_IMPLICIT], ids=lambda v: str(v))
def test_implicit_tracer_inputs_above_60_levels(L, nt):
    """test_gpu_tracer_column_shapes.py's smallplanet case in the implicit mode, the refused level count included (the oracle has no such
    limit): both calls return 0, stay finite (asserted in _oracle_calls) and change state and tracers."""
    g, rough, tr = tcs._case(L, nt)
    want = tcs._oracle_calls(L, nt, ("v_step_implicit", "v_step_implicit_terms_explicitly"))
    for st, t in want:
        assert 0.0 < max(tcs._errs(st, rough)) < float("inf") and 0.0 < max(tcs._terrs(t, tr)) < float("inf"), (L, nt)


@pytest.mark.parametrize("ud", [True, False], ids=["udiff", "plain"])
@pytest.mark.parametrize("L,nt", tcs.NEW_SHAPES + [tcs.REFUSED_VT_COLUMN], ids=lambda v: str(v))
def test_explicit_tracer_inputs_above_60_levels(L, nt, ud):
    """... and in the fully explicit mode at dt = 0.7, with and without uniform diffusion."""
    g, rough, tr = tcs._case(L, nt)
    want = tcs._oracle_calls(L, nt, ("v_step_explicit", "v_step_implicit_terms_explicitly"), fully_explicit=True, uniform_diffusion=tcs.UDIFF if ud else None)
    for st, t in want:
        assert 0.0 < max(tcs._errs(st, rough)) < float("inf") and 0.0 < max(tcs._terrs(t, tr)) < float("inf"), (L, nt, ud)


def test_whole_step_inputs_at_157_levels():
    """test_whole_steps_at_157_levels_vs_oracle's programs: every step returns 0, stays finite and changes the state."""
    from oracle_lib import Oracle
    L, _ = tcs.STEPS_SHAPE
    g, states = gu.make_grid(3, L, 6)
    o = Oracle(g, ninst=tcs.STEPS_NINST); o.set_state(0, states)
    assert o.step_ars343(100.0) == 0
    smooth = o.get_state(0)
    for prog in ([("ars343", False), ("ars343", False), ("strang", True)], [("ark232", False), ("ark232", False)]):
        o.set_state(0, smooth)
        for scheme, first in prog:
            before = o.get_state(0)
            assert o.step(scheme, 100.0, first=first) == 0, scheme
            assert _all_finite(o.get_state(0)) and 0.0 < max(gu.prognostic_errors(o.get_state(0), before)) < float("inf"), scheme
