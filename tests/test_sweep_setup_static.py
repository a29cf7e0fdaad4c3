"""The duo kernel's split row finish (duo_finish_rows, DESIGN section 4 "Helper wavefront") in the built gfx950 code object, no GPU
needed: both halves exist for both robots, fp32 only, hold no barrier (C2 is one more call of duo_join_rows), touch nothing but LDS,
spill nothing, and together are little longer than the phase_finish_team they stand in for.  The sweeps are not touched: every
pgs_team_variant keeps the parent's instructions outside its loop and its LDS reads there, to the instruction -- the partner-free
set-up that was to come with this change moved the step's bits on the GPU and is not in it (DESIGN, "Not taken")."""
import re

import pytest

from solorl_amd import build

# (LIM, NNS, NFS, CONE) of the K7 sweeps with contacts, pgs_team_variant<float, RowLds<float,4>, LIM, NNS, NFS, true, true, CONE>, on
# the build of the parent commit cafd9b5: (function body - loop span, ds_read outside the loop, loop span) by devcode.function_stats
# "body" and devcode.loop_stats.  The set-up's cost: what runs once per sub-step in front of the loop.
PARENT = {
    (0, 1, 1, 0): (295, 19, 101), (0, 1, 1, 1): (295, 19, 102), (0, 1, 2, 0): (378, 28, 127), (0, 1, 2, 1): (371, 28, 129),
    (0, 2, 3, 0): (561, 46, 175), (0, 2, 3, 1): (532, 46, 178), (0, 2, 4, 0): (655, 55, 200), (0, 2, 4, 1): (620, 55, 202),
    (0, 3, 5, 0): (855, 73, 246), (0, 3, 5, 1): (797, 73, 251), (0, 3, 6, 0): (972, 81, 273), (0, 3, 6, 1): (923, 81, 275),
    (0, 4, 7, 0): (1227, 100, 321), (0, 4, 7, 1): (1189, 100, 327), (0, 4, 8, 0): (1341, 108, 343), (0, 4, 8, 1): (1317, 108, 350),
    (1, 1, 1, 0): (379, 29, 125), (1, 1, 1, 1): (380, 29, 127), (1, 1, 2, 0): (467, 37, 150), (1, 1, 2, 1): (455, 37, 151),
    (1, 2, 3, 0): (658, 56, 197), (1, 2, 3, 1): (627, 56, 200), (1, 2, 4, 0): (743, 64, 223), (1, 2, 4, 1): (698, 64, 225),
    (1, 3, 5, 0): (980, 82, 271), (1, 3, 5, 1): (922, 82, 275), (1, 3, 6, 0): (1095, 91, 294), (1, 3, 6, 1): (1049, 91, 300),
    (1, 4, 7, 0): (1341, 109, 343), (1, 4, 7, 1): (1325, 109, 349), (1, 4, 8, 0): (1465, 118, 368), (1, 4, 8, 1): (1453, 118, 373),
}
# duo_finish_rows<SECOND = false> + <SECOND = true> against phase_finish_team (468, tests/test_helper_wave_static.py).  Each half repeats
# what phase_finish_team does once for its two rows -- the prologue, the team's counts, the 36 + 6 reads of the base-solve block, the
# empty-position test -- and issues one row's emit: the build gives 260 + 250 = 510, 42 above.  Neither half is on the other's path:
# what the main wavefront runs between barriers C and C2 is the first alone.
FINISH_PARENT, FINISH_MARGIN = 468, 45


@pytest.fixture(scope="module")
def code():
    from solorl_amd import devcode
    build.build()
    text = devcode.disassemble(build.LIB)
    stats = devcode.function_stats(build.LIB)
    rows = devcode._function_rows(text, "pgs_team_variantIfNS")
    sweeps = {}
    for n, s in devcode.loop_stats(build.LIB, "pgs_team_variantIfNS", text=text).items():
        lim, nn, nf, early, pipe, cone = (int(x) for x in re.search(r"Li(\d)ELi(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)EEE", n).groups())
        if early and nn + nf > 0:
            lo, hi = s["loop"]
            outside = [op for off, op in rows[n] if not lo <= off <= hi]
            sweeps[(lim, nn, nf, cone)] = (stats[n]["body"] - s["insts_in_loop"], sum(op.startswith("ds_read") for op in outside), s["insts_in_loop"])
    return sweeps, stats


def test_sweep_set_up_is_the_parents(code):
    sweeps, _ = code
    assert sorted(sweeps) == sorted(PARENT)
    for key, got in sorted(sweeps.items()):
        print(key, "outside the loop, ds_read there, loop span:", got, "parent", PARENT[key])
        assert got == PARENT[key], (key, got, PARENT[key])


@pytest.mark.parametrize("robot", [0, 1])
def test_finish_halves(code, robot):
    _, stats = code
    halves = []
    for second in (0, 1):
        hits = [n for n in stats if re.search(r"duo_finish_rowsIfLi%dE.*Lb%dEEE" % (robot, second), n)]
        assert len(hits) == 1, hits
        s = stats[hits[0]]
        print(hits[0][:90], s)
        assert s["barriers"] == 0 and s["scratch"] == 0 and s["flat"] == 0 and s["global"] == 0, (hits[0], s)
        halves.append(s["body"])
    finish = [n for n in stats if re.search(r"phase_finish_teamIfLi%dE" % robot, n)]
    assert len(finish) == 1 and stats[finish[0]]["body"] == FINISH_PARENT
    assert max(halves) < FINISH_PARENT                       # what the main wavefront runs between C and C2
    assert sum(halves) <= FINISH_PARENT + FINISH_MARGIN, (halves, FINISH_PARENT)
    assert not [n for n in stats if "duo_finish_rowsId" in n]            # fp32 only


def test_the_new_barrier_is_a_call(code):
    """C2 is one more call of duo_join_rows by either role: the kernel body still holds four s_barrier (tests/test_helper_wave_static.py),
    duo_join_rows one"""
    _, stats = code
    for robot in (0, 1):
        join = [n for n in stats if re.search(r"duo_join_rowsIfLi%dE" % robot, n)]
        assert len(join) == 1 and stats[join[0]]["barriers"] == 1, join
        duo = [n for n in stats if re.search(r"duo_kernel_teamIfLi%dEEE" % robot, n)]
        assert len(duo) == 1 and stats[duo[0]]["barriers"] == 4, duo
