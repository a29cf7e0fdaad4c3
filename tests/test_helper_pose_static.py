"""Barriers D and Z of the helper wavefront (duo_kernel_team, DESIGN section 4 "Helper wavefront") in the built gfx950 code object, no
GPU needed.  Behind barrier D the integrate is split over the two wavefronts: duo_integrate_joints (main: impulse cache and joints) and
duo_integrate_base (helper: base pose and the next sub-step's R0), two non-inlined device functions, fp32 only.  Neither holds a barrier
-- D and Z are further calls of duo_join_rows by both roles -- and neither touches scratch; the duo kernel keeps its resource bounds.  A
mismatched barrier is a hang, so this runs before anything is launched."""
import re

import pytest

from solorl_amd import build

NEW = ("duo_integrate_joints", "duo_integrate_base")
HALVES = {0: (86, 200), 1: (88, 200)}      # robot: instructions (devcode.function_stats "body") of the two, in NEW's order


@pytest.fixture(scope="module")
def code():
    from solorl_amd import devcode
    build.build()
    return devcode.function_stats(build.LIB), devcode.kernel_resources(build.LIB), devcode.kernel_static_lds(build.LIB)


def _hits(stats, pattern):
    return [n for n in stats if re.search(pattern, n)]


@pytest.mark.parametrize("robot", [0, 1])
def test_new_functions_exist_for_fp32_only(code, robot):
    stats, res, _ = code
    for fn in NEW:
        hits = _hits(stats, r"solo\d+%sIfLi%dE" % (fn, robot))
        assert len(hits) == 1, (fn, hits)
        assert hits[0] not in res                                    # a device function, not a kernel
        assert not _hits(stats, r"%sId" % fn), fn                    # no fp64 instantiation
    assert len(_hits(stats, "|".join(NEW))) == 2 * len(NEW)          # robots 0 and 1, nothing else by these names


@pytest.mark.parametrize("robot", [0, 1])
def test_no_barrier_and_no_scratch(code, robot):
    stats, _, _ = code
    for fn in NEW:
        s = stats[_hits(stats, r"solo\d+%sIfLi%dE" % (fn, robot))[0]]
        print(fn, robot, s)
        assert s["barriers"] == 0 and s["scratch"] == 0, (fn, s)
        assert s["flat"] == 0 and s["global"] == 0, (fn, s)          # LDS only: the split moves no HBM traffic


@pytest.mark.parametrize("robot", [0, 1])
def test_the_split_is_no_second_integrate_phase(code, robot):
    """the classic phase keeps its one fp32 instantiation per robot (tests/test_helper_wave_static.py pins its instruction count: 253 /
    254), and the two halves are the sizes measured on this commit's build: the joints half 86 / 88 instructions, the base half 200
    (the leader block, quat_to_mat with its nine stores, the w loads a second time) -- a duplicated leader block or a lost load hoist
    would show here"""
    stats, _, _ = code
    whole = _hits(stats, r"phase_integrate_teamIfLi%dE" % robot)
    assert len(whole) == 1, whole
    bodies = tuple(stats[_hits(stats, r"solo\d+%sIfLi%dE" % (fn, robot))[0]]["body"] for fn in NEW)
    print(robot, stats[whole[0]]["body"], bodies)
    assert bodies == HALVES[robot], (bodies, HALVES[robot])


@pytest.mark.parametrize("robot", [0, 1])
def test_duo_kernel_resources(code, robot):
    """<= 256 VGPRs, no AGPRs, scratch no larger than the classic kernel's, no static LDS, with the new calls in the kernel's call graph"""
    _, res, lds = code
    duo = [n for n in res if re.search(r"duo_kernel_teamIfLi%dEEE" % robot, n)]
    classic = [n for n in res if re.search(r"16step_kernel_teamIfLi%dEEE" % robot, n)]
    assert len(duo) == 1 and len(classic) == 1
    d, c = res[duo[0]], res[classic[0]]
    assert d["vgpr_count"] <= 256 and d["agpr_count"] == 0, d
    assert d["private_segment_fixed_size"] <= c["private_segment_fixed_size"], (d, c)
    assert lds[duo[0]] == 0 and d["group_segment_fixed_size"] == 0, d
