"""The cells of tests/schemes_common.py are worth running: asserted here on the C oracle and on the library's host logic alone, no device.
Per cell (configuration x scheme, and the mixed sequence per configuration): the oracle returns 0 after every step, every compared value
is finite, every compared variable changes in every step, no two schemes give the same result in any compared variable (the scheme axis
is not empty), the last-step flag changes instance 1 of the five Strang schemes and nothing else, Strang's vertical filter acts where
there are tracers, and the interpreter expectations the GPU file asserts are definite."""
import pytest
import golden_util as gu
import tracer_inputs_common as tc
import schemes_common as sc

ALL_CONFIGS = sc.CONFIGS + sc.RANK_CONFIGS


@pytest.mark.parametrize("name", ALL_CONFIGS)
def test_every_cell_runs_finite_and_moves(name):
    """rc 0 and finite after every step; every compared variable of instance 0 changes in every step (the shallow-water state under all
    ten schemes, ARK232 included); Strang's carried instance is finite (it is what the closing column solve changed: its U, V are zero,
    and all of it where that solve does nothing)."""
    sw = name == "sw"
    start = (sc.config(name)[1], sc.config(name)[2])
    for scheme in sc.SCHEMES:
        snaps, rcs = sc.want(name, scheme)
        assert rcs == [0] * len(sc.SEQUENCE), (scheme, rcs)
        before = start
        for k, s in enumerate(snaps):
            for ix in sc.compared_instances(scheme):
                assert sc.finite(s[ix]), (scheme, k, ix)
            moved = sc.differences(s[0], before, sw)
            assert min(moved) > 0.0 and max(moved) < float("inf"), (scheme, k, moved)
            before = s[0]


@pytest.mark.parametrize("name", ALL_CONFIGS)
def test_no_two_schemes_agree_in_any_variable(name):
    """After every step, the results of any two schemes differ in every compared variable."""
    sw = name == "sw"
    for k in range(len(sc.SEQUENCE)):
        for i, a in enumerate(sc.SCHEMES):
            for b in sc.SCHEMES[i + 1:]:
                d = sc.differences(sc.want(name, a)[0][k][0], sc.want(name, b)[0][k][0], sw)
                assert min(d) > 0.0, (a, b, k, d)


@pytest.mark.parametrize("name", sc.CONFIGS)
def test_last_step_flag_changes_the_carried_instance_of_strang_alone(name):
    """After the fourth step (last = True) instance 0 is bit-equal to a run that never sets the flag, for all ten schemes; instance 1
    differs in every compared variable for the five Strang schemes (the closing LinearCombineData(m_dCarryoverFinal, 1) is left out)
    and is bit-equal for the other five.  The restart behind it (first = True: the carried instance is not read) ends bit-equal in
    instance 0 again."""
    sw = name == "sw"
    k = [last for _, last in sc.SEQUENCE].index(True)
    for scheme in sc.SCHEMES:
        with_flag, without = sc.want(name, scheme)[0], sc.want(name, scheme, flag=False)[0]
        assert max(sc.differences(with_flag[k][0], without[k][0], sw)) == 0.0, scheme
        d1 = sc.differences(with_flag[k][1], without[k][1], sw)
        if scheme in sc.STRANG:
            assert min(d1) > 0.0 and max(d1) < float("inf"), (scheme, d1)
        else:
            assert max(d1) == 0.0, (scheme, d1)
        assert max(sc.differences(with_flag[k + 1][0], without[k + 1][0], sw)) == 0.0, scheme


@pytest.mark.parametrize("name", ["jw_tr", "expl_udiff_tr", "jw_tr_p24"])
def test_strangs_vertical_filter_acts_on_steps_that_are_not_first(name):
    """The input of FilterNegativeTracers(0) at the head of a Strang step that is not a first one (TimestepSchemeStrang.cpp:476-481) is
    instance 0 + instance 1 of the step before: for every Strang scheme the filter changes at least one column in such a step of a cell, and
    columns of mixed sign whose r is not 1 occur (tracer_inputs_common.class_counts)."""
    g = sc.config(name)[0]
    for scheme in sc.STRANG:
        snaps = sc.want(name, scheme)[0]
        acted = []
        for k, (first, _) in enumerate(sc.SEQUENCE):
            if first:
                continue
            o = tc.oracle(g)
            o.set_tracers(0, snaps[k - 1][0][1]); o.set_tracers(1, snaps[k - 1][1][1])
            o.linear_combine_data([1.0, 1.0], 0)
            tin = o.get_tracers(0)
            o.filter_negative_tracers_v(0)
            tout = o.get_tracers(0)
            changed, r_not_1 = 0, 0
            for a, b in zip(tin, tout):
                cin, cout = tc.cells(a, True), tc.cells(b, True)
                changed += int((cin != cout).any(1).sum())
                r_not_1 += tc.class_counts(cin, cout)["r != 1"]
            print("%s %s step %d: %d columns changed by the vertical filter, %d of mixed sign with r != 1" % (name, scheme, k + 1, changed, r_not_1))
            acted.append(min(changed, r_not_1))
        # with implicit vertical dynamics in all three such steps; in the fully explicit mode the carried instance is zero and the input
        # is the filtered state of the step before: by the third step no column holds a negative value any more
        assert max(acted) >= 1 and (min(acted) >= 1 or name == "expl_udiff_tr"), (scheme, acted)


@pytest.mark.parametrize("name", sc.MIXED_CONFIGS)
def test_mixed_sequence_runs_finite_and_moves(name):
    start = (sc.config(name)[1], sc.config(name)[2])
    snaps, rcs = sc.want_mixed(name)
    assert rcs == [0] * len(sc.MIXED_SEQUENCE), rcs
    before = start
    for k, ((scheme, _, _), s) in enumerate(zip(sc.MIXED_SEQUENCE, snaps)):
        for ix in sc.compared_instances(scheme):
            assert sc.finite(s[ix]), (k, scheme, ix)
        assert min(sc.differences(s[0], before)) > 0.0, (k, scheme)
        before = s[0]


def test_interpreter_expectations_are_definite():
    """What the GPU file asserts through tmx_info, from the host logic alone: every program has a node-unique form; with a Rayleigh layer
    the Strang family stays element-major and ARS232 / ARS443 are decided by the data; the in-patch copies of the 6-patch grids agree in
    the geometry ARK232's terms kernel reads (so ARK232 runs node-unique there), those of ne6 on 24 patches do not; ARS343's stored prefix
    exists on every kind of step."""
    for scheme in sc.SCHEMES:
        for first, last in set(sc.SEQUENCE):
            assert sc.has_unique_form(scheme, first, last), (scheme, first, last)
            assert sc.keeps_unique_with_rayleigh(scheme, first, last) == (scheme not in sc.STRANG), scheme
            assert sc.reads_copy_by_copy(scheme, first, last) == (scheme in ("ars343", "ars222", "ark232")), scheme
            assert sc.expect_unique("jw_tr", scheme, first, last) is False and sc.expect_unique("sw", scheme, first, last) is False
            want = {s: False for s in sc.STRANG}
            want.update(ars232=None, ars443=None)
            assert sc.expect_unique("schar", scheme, first, last) is want.get(scheme, True), scheme
            assert sc.expect_unique("jw", scheme, first, last) is True and sc.expect_unique("visc0", scheme, first, last) is True
    for name in sc.UNIQUE_CONFIGS:
        assert sc.vite_copies_agree(name), name
    assert not sc.grid_copies_agree(gu.make_grid(6, 6, 24)[0])      # (a grid on which they do not: ARK232 runs element-major there)
    for first, last in set(sc.SEQUENCE):
        assert sc.prefix_pairs("ars343", first, last) == 1
    assert [sc.expect_mixed_steps("schar", "ars343", k) for k in range(5)] == [1, 2, 3, 4, 5]
    assert [sc.expect_mixed_steps("jw", "ars222", k) for k in range(5)] == [1] * 5
    assert [sc.expect_mixed_steps("jw", "strang", k) for k in range(5)] == [0] * 5 and sc.expect_mixed_steps("schar", "ars232", 3) == 0


def test_rank_grid_is_the_smallest_with_early_and_late_tiles():
    """ne10 on 24 patches: every rank of three owns tiles of both kinds (plan-only engines: the tile lists of a boundary-first stage);
    at ne8 and below on 24 patches no rank does, so the stages would not split."""
    from tempestmodel_amd.engine import Engine
    for ne, split in ((sc.RANKS_NE - 2, False), (sc.RANKS_NE, True)):
        g = sc.config("jw_p24")[0] if ne == sc.RANKS_NE else gu.make_grid(ne, 5, 24)[0]
        for r in range(sc.N_RANKS):
            e = Engine(g, rank=r, n_ranks=sc.N_RANKS, n_instances=sc.NINST, device=-2)
            try:
                early, late = len(e.plan(7)), len(e.plan(8))
            finally:
                e.close()
            assert (early > 0 and late > 0) == split, (ne, r, early, late)
