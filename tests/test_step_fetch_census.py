"""What the compiler makes of a traversal step whose rare half requests no record and has none requested ahead of it -- NOT one request per
step on every instantiation: with the tree in HBM node_step still requests in the steps the rare half does not follow (Tracer::step, DESIGN.md 5.8;
tools/loop_census.py run on the tree this file is in, ~20 s).  Same form as tests/test_slow_step_census.py, whose ceilings stay in force: the
figures here are what the build reaches, each at or below the ceiling that file holds for it.

Before, node_step always ended with a request for the node lanes, and slow_step with another for the lanes that had popped; the compiler
tracks the record registers, not lanes, so the leaf test opened with an s_waitcnt vmcnt(0) that made the leaf lanes wait for the node lanes'
fresh request, and the poppers' request was a second latency in the same step.  Now, with the tree in LDS, every step requests ONCE, at its
end, for the lanes that either half moved.  With the tree in HBM a step that the rare half follows requests once, behind it, for every lane;
a step that it does not follow requests in node_step as before, ahead of the deep-stack reload (with one request site for both kinds of
step the reload's latency and the record's came one after the other in every step with a deep pop: measured, 5.8).  So the burst loop of the
instantiations that read the tree from HBM holds two rows of four global_load_dwordx4 -- node_step's and the one behind the rare step --
and none inside the pop loop; a tree in LDS is read with ds_read and has none.
Ordinary opcodes are counted, nothing else is looked for."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# instantiation: (burst loop: instructions, branches, moves; pop loop: instructions, moves, branches)
FIGURES = {
    "<false,false,8>": (334, 21, 17, 24, 0, 3),
    "<false,true,4>": (320, 22, 17, 24, 0, 3),
    "<false,true,8>": (320, 22, 17, 24, 0, 3),
    "<true,false,8>": (336, 22, 17, 24, 0, 3),
    "<true,true,4>": (321, 22, 17, 24, 0, 3),
    "<true,true,8>": (321, 22, 17, 24, 0, 3),
}
HBM = ("<false,false,8>", "<true,false,8>")


@pytest.fixture(scope="module")
def census():
    import loop_census
    result = loop_census.run()
    print(loop_census.table(result))
    return result


def test_figures_are_at_or_below_the_existing_ceilings():
    from tests.test_slow_step_census import CEILINGS
    assert sorted(FIGURES) == sorted(CEILINGS)
    for name, (instructions, branches, moves, pop_instructions, pop_moves, _) in FIGURES.items():
        assert all(a <= b for a, b in zip((instructions, branches, moves, pop_instructions, pop_moves), CEILINGS[name])), name


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_burst_loop_holds_its_figures(census, name):
    instructions, branches, moves, pop_instructions, pop_moves, pop_branches = FIGURES[name]
    burst, pop = census[name]["burst"], census[name]["pop"]
    assert burst["instructions"] <= instructions, burst
    assert burst["branches"] <= branches, burst
    assert burst["moves"] <= moves, burst
    assert burst["scratch"] == 0 and burst["lane_reads"] == 0 and burst["lane_writes"] == 0 and burst["flat_loads"] == 0, burst
    assert pop["instructions"] <= pop_instructions and pop["moves"] <= pop_moves and pop["branches"] <= pop_branches, pop


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_record_requests_of_a_step(census, name):
    """A tree in HBM: two rows of four global_load_dwordx4 in the burst loop (node_step's, and the one behind the rare step), none of them
    in the pop loop; a tree in LDS: no such load."""
    burst, pop, rows = census[name]["burst"], census[name]["pop"], census[name]["record_groups"]
    assert pop["record_loads"] == 0, pop
    if name in HBM:
        assert rows == [4, 4], rows
        assert burst["record_loads"] == 8, burst
    else:
        assert rows == [] and burst["record_loads"] == 0, (rows, burst)


def test_record_rows_are_counted_as_rows():
    import loop_census
    load = "global_load_dwordx4 v[4:7], v[20:21], off"
    assert loop_census._record_groups([load, load, load, "s_nop 0", load, "s_waitcnt vmcnt(0)", load, "v_mov_b32 v0, v1", load, load]) == [4, 1, 2]
    assert loop_census._record_groups(["s_nop 0", "v_add_f32 v0, v1, v2"]) == []
    assert loop_census._count([load, "global_load_dwordx2 v[0:1], v[2:3], off"])["record_loads"] == 1


def test_table_has_the_new_column(census):
    import loop_census
    assert loop_census.COLUMNS[-1] == "record_loads"
    head = loop_census.table(census).splitlines()[0].split()
    assert head == ["instantiation", "region"] + list(loop_census.COLUMNS)
