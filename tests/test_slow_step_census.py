"""Ceilings on what the compiler makes of the rare step inside the path kernel's burst loop (tools/loop_census.py, run on the tree this file
is in; ~20 s).  Same form and purpose as tests/test_path_loop_census.py, which pins the code around the burst loop and the loop's total.

Tracer::slow_step -- the leaf test, what follows a hit, the pop loop -- runs for the few lanes that wait for it while the rest of the wavefront
stands still, and on the benchmark frame it is a fifth of a wavefront's life (profiles/slow_step_share.txt).  Its parent compiled to
(all six instantiations alike but for the loop's total)

    burst loop   413 / 409 / 409 / 415 / 409 / 409 instructions, 37 branches, 20 VGPR-to-VGPR moves
    pop loop     48 instructions, 6 branches, 4 moves: every trip copied the walk's `cur` and `sp` to other registers and back

-- sixteen divergent regions from the early returns of the triangle test and the nested tests behind it, and a pop loop with a flag beside
`cur` and several ways round.  As straight-line code with selects, and a pop loop that carries `sp` and `cur` alone with one test at its
bottom: the figures below.  They keep the branches and the moves from growing back; lower them when a change removes more.
Ordinary opcodes are counted, nothing else is looked for."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# instantiation: (burst loop: instructions, branches, moves; pop loop: instructions, moves)
CEILINGS = {
    "<false,false,8>": (334, 22, 17, 24, 0),
    "<false,true,4>": (330, 22, 17, 24, 0),
    "<false,true,8>": (330, 22, 17, 24, 0),
    "<true,false,8>": (336, 23, 17, 24, 0),
    "<true,true,4>": (332, 23, 17, 24, 0),
    "<true,true,8>": (332, 23, 17, 24, 0),
}
# the parent's burst loop: instructions, branches, moves -- every ceiling above is below its figure
PARENT = {
    "<false,false,8>": (413, 37, 20),
    "<false,true,4>": (409, 37, 20),
    "<false,true,8>": (409, 37, 20),
    "<true,false,8>": (415, 37, 20),
    "<true,true,4>": (409, 37, 20),
    "<true,true,8>": (409, 37, 20),
}
PARENT_POP = (48, 4)


@pytest.fixture(scope="module")
def census():
    import loop_census
    result = loop_census.run()
    print(loop_census.table(result))
    return result


def test_ceilings_are_below_the_parent():
    assert sorted(CEILINGS) == sorted(PARENT)
    for name, (instructions, branches, moves, pop_instructions, pop_moves) in CEILINGS.items():
        assert instructions < PARENT[name][0] and branches < PARENT[name][1] and moves < PARENT[name][2], name
        assert pop_instructions < PARENT_POP[0] and pop_moves < PARENT_POP[1], name


def test_every_instantiation_has_a_pop_loop(census):
    assert sorted(census) == sorted(CEILINGS)
    for name in census:
        assert census[name]["pop"]["instructions"] > 0 and census[name]["loops"]["pop"] != census[name]["loops"]["burst"], census[name]["loops"]


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_burst_loop(census, name):
    instructions, branches, moves, _, _ = CEILINGS[name]
    c = census[name]["burst"]
    assert c["instructions"] <= instructions, c
    assert c["branches"] <= branches, c
    assert c["moves"] <= moves, c


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_pop_loop(census, name):
    _, _, _, instructions, moves = CEILINGS[name]
    c = census[name]["pop"]
    assert c["instructions"] <= instructions, c
    assert c["moves"] <= moves, c  # no copy of the walk's state inside the loop
    assert c["instructions"] <= census[name]["burst"]["instructions"]  # (the pop loop is part of the burst loop)
