"""All ten time schemes against the C oracle in every configuration that changes what tmx_step runs on the device: the cells, inputs and
interpreter expectations of tests/schemes_common.py (its header holds the table and the cells that fall back by design), qualified on the
CPU by tests/test_schemes_inputs_host.py.  What combines the kernels -- build_program, the matcher of fused units, the copy sharing, the
stored prefix, the boundary-first stages and both interpreters (tmx_program.hip) -- is compared here with the oracle's call-for-call
statement of the reference's Step functions, bit for bit (parity_common.EXACT), after EVERY step of: a first step, two plain steps, a step
with the last-step flag, and a first step again (a run restarted on the same engine); instance 0 with its tracers, and the carried
instance 1 of the five Strang schemes.

Which interpreter ran is asserted through tmx_info against expectations restated from the library's host logic (tmx_debug_program_*) and
the grid's arrays on the CPU, never read back from the engine under test.

Shown to bite (a scratch build each, one GPU run of this file each):
    * build_program without the `if (!last)` in front of Strang's closing LinearCombineData(m_dCarryoverFinal, 1): the fourth step of every
      Strang cell fails in instance 1 (relative difference about 1 in rho*theta, W, rho and exactly 1 in U, V) -- all 80 of them, both
      layouts, ranks and graph replay included -- and the seventh step of the mixed sequence in its four variants: 84 of 164 tests.  The
      stepper-facing GPU tests that existed before (test_gpu_steppers, _unique_layout, _multirank_loopback, _two_process, _adapter and the
      other files from m on) all pass with that library;
    * the third combination of strang_ssprk53 with its first coefficient 0.762406163401431 written 0.762406163401432: every strang_ssprk53 cell
      fails at its first step (differences of 1e-15, W 3e-14), the mixed sequence at its last: 20 of 164.  Before, one test saw it:
      test_strang_explicit_discretisations[strang_ssprk53] on ne2 L4 in the default configuration."""
import pytest
import golden_util as gu
import schemes_common as sc
from parity_common import EXACT, _rank_engines_step, INFO_EARLY_TILES, INFO_LATE_TILES

pytestmark = pytest.mark.gpu

INFO_UNIQUE_LAYOUT, INFO_UNIQUE_INSTANCES, INFO_PREFIX_STAGES, INFO_MIXED_STEPS = 12, 13, 17, 19


def _engine(name, options=None, **more):
    from tempestmodel_amd.engine import Engine
    g, st, tr, kw, _ = sc.config(name)
    e = Engine(g, n_instances=sc.NINST, options=options, **kw, **more)
    try:
        e.upload_state(0, st)
        if tr is not None:
            e.upload_tracers(0, tr)
    except Exception:
        e.close()
        raise
    return e


def _compare(e, want, instances, what):
    """The engine's instances against the oracle's snapshots on the patches the engine owns, at the exact bar; a non-finite value on
    either side is a failure (golden_util's helpers)."""
    e.sync()
    own = e.local_patches
    for ix in instances:
        st, tr = want[ix]
        got = e.download_state(ix)
        errs = gu.prognostic_errors([got[p] for p in own], [st[p] for p in own])
        assert max(errs) <= EXACT, (what, "instance", ix, "state", errs)
        if tr is not None:
            gt = e.download_tracers(ix)
            terr = gu.tracer_errors([gt[p] for p in own], [tr[p] for p in own])
            assert max(terr) <= EXACT, (what, "instance", ix, "tracers", terr)


def _run_cell(e, name, scheme, layout=None):
    """SEQUENCE on one engine against sc.want; layout 1 / 0: also the interpreter expectations of the module's header."""
    dt = sc.config(name)[4]
    snaps, rcs = sc.want(name, scheme)
    assert rcs == [0] * len(sc.SEQUENCE)
    mixed_before = 0
    for k, (first, last) in enumerate(sc.SEQUENCE):
        prefix_before = e.info(INFO_PREFIX_STAGES)
        e.step(scheme, dt, first=first, last=last)
        what = (name, scheme, "step %d" % (k + 1))
        if layout == 1:
            unique = sc.expect_unique(name, scheme, first, last)
            mixed = sc.expect_mixed_steps(name, scheme, k)
            pairs = sc.prefix_pairs(scheme, first, last)
            made = e.info(INFO_PREFIX_STAGES) - prefix_before
            if unique is False:
                assert e.info(INFO_UNIQUE_INSTANCES) == 0 and made == 0, what
            elif unique is True and (k >= 1 or mixed > mixed_before):
                assert e.info(INFO_UNIQUE_INSTANCES) > 0, what + ("did not run on the node-unique layout",)
                # a stage that read the element-major model state copy by copy stores no prefix; every other one the host logic plans does
                assert (0 <= made <= pairs) if mixed > mixed_before else made == pairs, what + (made, pairs)
            else:
                assert 0 <= made <= pairs, what + (made, pairs)
            assert e.info(INFO_MIXED_STEPS) == mixed, what
            mixed_before = mixed
        elif layout == 0:
            assert e.info(INFO_UNIQUE_INSTANCES) == 0 and e.info(INFO_PREFIX_STAGES) == 0 and e.info(INFO_MIXED_STEPS) == 0, what
        _compare(e, snaps[k], sc.compared_instances(scheme), what)


CELLS = [(name, scheme, layout) for name in sc.CONFIGS for layout in ((1, 0) if name in sc.UNIQUE_CONFIGS else (None,)) for scheme in sc.SCHEMES]


def _cell_id(c):
    return "%s-%s%s" % (c[0], c[1], "" if c[2] is None else "-unique%d" % c[2])


@pytest.mark.parametrize("name,scheme,layout", CELLS, ids=[_cell_id(c) for c in CELLS])
def test_cell_against_the_oracle(name, scheme, layout):
    """One engine, one cell.  The configurations eligible for the node-unique layout run with the option on and off, BOTH against the oracle;
    the others must not have built the layout."""
    e = _engine(name, options=None if layout is None else {"unique_layout": layout})
    try:
        assert e.info(INFO_UNIQUE_LAYOUT) == (1 if layout == 1 else 0), (name, layout)
        _run_cell(e, name, scheme, layout)
    finally:
        e.close()


@pytest.mark.parametrize("scheme", sc.SCHEMES)
@pytest.mark.parametrize("name", sc.RANK_CONFIGS)
def test_cell_on_three_rank_engines(name, scheme):
    """ne10 on 24 patches (the smallest such grid on which every rank of three owns early and late tiles: 5 x 5 elements per patch): the
    cell on one engine first, then -- only if that passed: a rank that raises leaves the others at a barrier -- on three loopback rank
    engines whose stages run boundary tiles first, every rank's own patches against the oracle after every step."""
    from tempestmodel_amd.engine import Engine
    dt = sc.config(name)[4]
    snaps, _ = sc.want(name, scheme)
    single = _engine(name)
    try:
        _run_cell(single, name, scheme)
    finally:
        single.close()
    ranks = []
    try:
        for r in range(sc.N_RANKS):
            ranks.append(_engine(name, rank=r, n_ranks=sc.N_RANKS))
        assert all(e.info(INFO_EARLY_TILES) > 0 and e.info(INFO_LATE_TILES) > 0 for e in ranks), [(e.info(INFO_EARLY_TILES), e.info(INFO_LATE_TILES)) for e in ranks]
        assert sorted(p for e in ranks for p in e.local_patches) == list(range(24))
        Engine.loopback_group(ranks)
        for k, (first, last) in enumerate(sc.SEQUENCE):
            _rank_engines_step(ranks, lambda e, _k: e.step(scheme, dt, first=first, last=last), 1)
            for e in ranks:
                _compare(e, snaps[k], sc.compared_instances(scheme), (name, scheme, "rank %d" % e.rank, "step %d" % (k + 1)))
        Engine.loopback_dissolve(ranks[0])
    finally:
        for e in ranks:
            e.close()


@pytest.mark.parametrize("scheme", sc.SCHEMES)
@pytest.mark.parametrize("name", sc.GRAPH_CONFIGS)
def test_cell_replayed_from_captured_graphs(monkeypatch, name, scheme):
    """TMX_GRAPH=1 (the option of test_graph_replay_is_bit_identical): every step of the cell is captured as a hipGraph keyed by (scheme,
    first, last, dt) and launched; the third step replays the second one's graph, the fifth the first one's, and a Strang cell holds
    three different programs.  Against the oracle, one engine per cell."""
    monkeypatch.setenv("TMX_GRAPH", "1")
    e = _engine(name)
    try:
        assert e.get_option("step_graph") == 1 and e.info(INFO_UNIQUE_LAYOUT) == 0
        _run_cell(e, name, scheme)
    finally:
        e.close()


MIXED = [("jw", 1), ("jw", 0), ("jw_tr", None), ("expl_udiff_tr", None)]


@pytest.mark.parametrize("name,layout", MIXED, ids=["%s%s" % (n, "" if l is None else "-unique%d" % l) for n, l in MIXED])
def test_mixed_sequence_of_schemes_on_one_engine(name, layout):
    """sc.MIXED_SEQUENCE on ONE engine against one oracle: every program starts from the slot sharing, the shared U,V slabs and the
    node-unique / element-major forms another scheme's program left behind."""
    dt = sc.config(name)[4]
    snaps, rcs = sc.want_mixed(name)
    assert rcs == [0] * len(sc.MIXED_SEQUENCE)
    e = _engine(name, options=None if layout is None else {"unique_layout": layout})
    try:
        assert e.info(INFO_UNIQUE_LAYOUT) == (1 if layout == 1 else 0)
        for k, (scheme, first, last) in enumerate(sc.MIXED_SEQUENCE):
            e.step(scheme, dt, first=first, last=last)
            if layout == 1 and k >= 1:      # (grid "jw": every program has a node-unique form, ARK232's included)
                assert sc.expect_unique(name, scheme, first, last) is True and e.info(INFO_UNIQUE_INSTANCES) > 0, (k, scheme)
            _compare(e, snaps[k], sc.compared_instances(scheme), (name, "mixed step %d" % (k + 1), scheme))
    finally:
        e.close()
