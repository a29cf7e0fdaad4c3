"""What one sweep of the K7 team sweeps issues, from the built gfx950 code object (no GPU needed).

A lone wavefront pays ~4 cycles for every instruction it issues, whatever the instruction does, and the launch lasts as long as the
wavefront that runs the heaviest sweep loop 50 x 4 times: the loop's instruction count IS the launch time ("Issue
slots per sweep").  `devcode.loop_stats` counts every instruction between the loop's branch targets -- the cold blocks that publish a
team's result lie inside that span, so the figures are ~45 above the common path; differences are what matters."""
import re

import pytest

from solorl_amd import build

# (LIM, NNS, NFS, CONE) of pgs_team_variant<float, RowLds<float,4>, LIM, NNS, NFS, EXIT = true, PIPE = true, CONE>:
#   (insts_in_loop, s_nop_in_loop) as measured on the build of the commit that added this file,
#   (insts_in_loop, s_nop_in_loop) of its parent 17b5093, same counting function
MEASURED = {
    (0, 1, 1, 0): (101, 3, 106, 1),
    (0, 1, 1, 1): (101, 0, 110, 2),
    (0, 1, 2, 0): (127, 3, 132, 1),
    (0, 1, 2, 1): (128, 1, 139, 2),
    (0, 2, 3, 0): (175, 3, 179, 0),
    (0, 2, 3, 1): (177, 1, 190, 2),
    (0, 2, 4, 0): (200, 4, 203, 0),
    (0, 2, 4, 1): (201, 1, 218, 3),
    (0, 3, 5, 0): (246, 2, 251, 0),
    (0, 3, 5, 1): (249, 0, 271, 5),
    (0, 3, 6, 0): (273, 4, 276, 0),
    (0, 3, 6, 1): (274, 0, 301, 7),
    (0, 4, 7, 0): (321, 4, 324, 0),
    (0, 4, 7, 1): (325, 2, 353, 8),
    (0, 4, 8, 0): (343, 2, 348, 0),
    (0, 4, 8, 1): (349, 2, 378, 6),
    (1, 1, 1, 0): (125, 2, 131, 1),
    (1, 1, 1, 1): (126, 0, 134, 1),
    (1, 1, 2, 0): (150, 3, 154, 0),
    (1, 1, 2, 1): (150, 0, 160, 0),
    (1, 2, 3, 0): (197, 2, 202, 0),
    (1, 2, 3, 1): (199, 0, 214, 3),
    (1, 2, 4, 0): (223, 3, 227, 0),
    (1, 2, 4, 1): (224, 0, 243, 4),
    (1, 3, 5, 0): (271, 3, 275, 0),
    (1, 3, 5, 1): (273, 0, 295, 5),
    (1, 3, 6, 0): (294, 2, 299, 0),
    (1, 3, 6, 1): (299, 2, 324, 7),
    (1, 4, 7, 0): (343, 3, 347, 0),
    (1, 4, 7, 1): (347, 1, 374, 6),
    (1, 4, 8, 0): (368, 3, 372, 0),
    (1, 4, 8, 1): (372, 1, 403, 7),
}
HEAVY = (1, 4, 8, 1)
# The plan was 35 fewer for the heaviest variant.  Five of them cannot be had: the loop-carried copies of the limit and normal rows'
# impulses (`del = sv - lm` needs the old and the new impulse at once; only unrolling the sweep by two frees them, and that doubles the
# loop, which tests/test_abi.py bounds).  Hence 30.
MIN_DROP_HEAVY = 30


@pytest.fixture(scope="module")
def sweeps():
    from solorl_amd import devcode
    build.build()
    out = {}
    for n, s in devcode.loop_stats(build.LIB, "pgs_team_variantIfNS").items():
        m = re.search(r"Li(\d)ELi(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)EEE", n)
        lim, nn, nf, early, pipe, cone = (int(x) for x in m.groups())
        if early and nn + nf > 0:
            assert pipe == 1, n                      # (the K7 sweeps are always pipelined)
            out[(lim, nn, nf, cone)] = s
    return out


def test_every_k7_sweep_with_contacts_is_in_the_table(sweeps):
    assert sorted(sweeps) == sorted(MEASURED)
    assert len(sweeps) == 32                         # {limit slot or not} x {1..8 contacts} x {pyramid, cone}


def test_sweep_loops_issue_no_more_than_measured(sweeps):
    for key, s in sorted(sweeps.items()):
        assert s["loop"][0] is not None, key
        print(key, s["insts_in_loop"], s["s_nop_in_loop"], "measured / parent", MEASURED[key])
        assert s["insts_in_loop"] <= MEASURED[key][0] * 1.02, (key, s, MEASURED[key])


def test_heaviest_sweep_dropped_its_non_arithmetic_slots(sweeps):
    s, (_, _, parent, parent_nop) = sweeps[HEAVY], MEASURED[HEAVY]
    print("heaviest K7 sweep: %d instructions in the loop span (%d s_nop); parent 17b5093: %d (%d s_nop)"
          % (s["insts_in_loop"], s["s_nop_in_loop"], parent, parent_nop))
    assert parent == 403
    assert s["insts_in_loop"] <= parent - MIN_DROP_HEAVY, (s, parent)
