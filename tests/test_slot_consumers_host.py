"""The inputs of tests/test_gpu_slot_consumers.py in its crafted slots, judged without a GPU: what keeps a case of
slam2d_refine_poses, slam2d_search_points, slam2d_refine_points and slam2d_mcl_step_adaptive from being vacuous there
(``conditions`` of that file) is computed with the yardsticks and NumPy's cos / sin on the crafted images, which are host arrays
(crafted_slot of tests/test_gpu_field_slots.py).  The device's cos / sin differ from NumPy's in a last bit here and there; the
conditions count beams, winners, bins and survivors and have room for that, and the GPU file asserts them again on the device's
values.  The input builders are that file's, not restated: a change to CRAFTED or slot_inputs that makes a case vacuous fails
here."""
import numpy as np
import pytest

import mcl_yardstick as mcl
import refine_yardstick as ryard
import test_gpu_field_slots as tslots
import test_gpu_slot_consumers as tcons
from test_gpu_field_slots import CRAFTED, FMAX, P
from test_score_host import walk


@pytest.fixture(scope="module")
def cases():
    """The crafted slots and their cases as the GPU file forms them, but for the cos / sin."""
    _, poses, scans = walk()                                   # world 0 of the level of three: its walk and scans
    scale, free = tcons.level_constants()
    slots = [tslots.crafted_slot(p, poses, scans) for p in range(P)]
    assert [s["size"] for s in slots] == [(FMAX, FMAX), (37, 101), (1, 1)] and [s["frame"] for s in slots] == [c[:2] for c in CRAFTED]
    return tcons.cases_of(slots, scale, free, mcl.numpy_sincos, built=False)


@pytest.mark.parametrize("call", tcons.CALLS)
@pytest.mark.parametrize("p", range(P))
def test_a_crafted_case_is_not_vacuous(cases, p, call):
    tcons.conditions(call, cases[p], mcl.numpy_sincos)


def test_the_sizes_are_the_smallest_that_still_turn_the_slot_arithmetic(cases):
    for p, c in enumerate(cases):
        ci = c["ci"]
        assert (ci["N"], ci["n_cap"]) == (70, 98) and np.isnan(ci["cloud"][70:]).all() and not np.isnan(ci["cloud"][:70]).any()
        assert ci["pts"].shape == (100, 2) and ci["sets"].shape == (len(ci["seeds"]), 100, 2) and ci["lat"][:3] == (5, 4, 8)
        assert len(ci["seeds"]) == (32 if p == 2 else 16) and ci["scans"].shape == (len(ci["seeds"]), tcons.BEAMS)
        assert c["outside"] not in (0, tcons.level_constants()[1], *tslots.POISON)       # neither a wall, free space nor a poison
    one = cases[2]["ci"]                                       # the frame of one cell: seeds within 0.4 m of it, ranges below 0.3 m
    xlo, ylo = CRAFTED[2][:2]
    assert (np.abs(one["seeds"][:, :2] - (xlo + 0.05, ylo + 0.05)) < 0.45).all() and one["scans"].max() < 0.3
    # most winners are another candidate than the seed, in every slot
    for c in cases:
        for call in ("refine_poses", "refine_points"):
            assert (ryard.index_of(c["want"][call][0]) != 0).mean() > 0.5, (c["p"], call)
