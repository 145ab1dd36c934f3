"""Ceilings on what the compiler makes of the path kernel's inner loop (tools/loop_census.py, run on the tree this file is in; ~20 s).

The code between two bursts of traversal steps -- retire, pass trigger, hand-out, Tracer::start, window reload -- used to be one third
register shuffling: the walk and its record lived in one set of vector registers inside the burst loop and in another outside it, and every
trip copied all 23 of them across and back (and waited for the records in flight to do so); the ring's window came back through flat
loads.  The parent of the change that removed this measured, per instantiation <wide slot word, records in LDS, stack window>
(VGPR-to-VGPR moves / v_readlane ahead of the burst loop; moves / v_readlane behind it; instructions of the burst loop):

    <false,false,8>  123 / 32   40 / 0   416        <true,false,8>  123 / 32   40 / 0   418
    <false,true,4>   123 / 29   40 / 0   410        <true,true,4>   123 / 31   40 / 0   412
    <false,true,8>   123 / 29   40 / 0   410        <true,true,8>   123 / 31   40 / 0   412

with two flat loads ahead of the burst loop in each.  (Counting every v_mov, constants included, and the loop's exit blocks with the
region behind the burst loop, <false,false,8> reads 132 / 32 and 47 / 8.)  The change reached 19 moves and 11-14 lane reads ahead of the
burst loop, none behind it, no flat load, and burst loops of 409-415 instructions (profiles/refill_census.txt).  The
ceilings below are those figures: they keep the moves and the lane reads from growing back, as MAX_VGPR_SPILLS of
tests/test_kernel_resources.py does for spills.  Lower them when a change removes more."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# instantiation: (moves ahead, lane reads ahead, moves behind, lane reads behind, instructions of the parent's burst loop)
CEILINGS = {
    "<false,false,8>": (19, 14, 0, 0, 416),
    "<false,true,4>": (19, 12, 0, 0, 410),
    "<false,true,8>": (19, 12, 0, 0, 410),
    "<true,false,8>": (19, 13, 0, 0, 418),
    "<true,true,4>": (19, 11, 0, 0, 412),
    "<true,true,8>": (19, 11, 0, 0, 412),
}


@pytest.fixture(scope="module")
def census():
    import loop_census
    result = loop_census.run()
    print(loop_census.table(result))
    return result


def test_every_instantiation_is_found(census):
    assert sorted(census) == sorted(CEILINGS)


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_no_flat_load_outside_the_bursts(census, name):
    assert census[name]["ahead"]["flat_loads"] == 0 and census[name]["behind"]["flat_loads"] == 0, census[name]


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_moves_and_lane_reads_do_not_grow_back(census, name):
    moves_ahead, reads_ahead, moves_behind, reads_behind, _ = CEILINGS[name]
    c = census[name]
    assert c["ahead"]["moves"] <= moves_ahead, c["ahead"]
    assert c["ahead"]["lane_reads"] <= reads_ahead, c["ahead"]
    assert c["behind"]["moves"] <= moves_behind, c["behind"]
    assert c["behind"]["lane_reads"] <= reads_behind, c["behind"]


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_burst_loop_did_not_grow(census, name):
    assert census[name]["burst"]["instructions"] <= CEILINGS[name][4], census[name]["burst"]
