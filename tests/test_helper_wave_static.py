"""The helper-wavefront kernels (duo_kernel_team, DESIGN section 4 "Helper wavefront") in the built gfx950 code object, no GPU needed:
they exist, keep the step kernels' resource bounds, hold exactly the documented workgroup barriers -- a mismatched barrier is a hang --
and the classic kernels and phases beside them are the code they were before the helper existed."""
import re

import pytest

from solorl_amd import build

# instructions of the classic team-mode kernels and phase instantiations (devcode.function_stats "body": up to the function's last
# instruction, without the s_nop run that pads it to the next symbol), measured on the build of the parent commit ca34e8a.
# (T, robot): step_kernel_team, rollout_kernel_team
PARENT_KERNELS = {("f", 0): (8450, 9939), ("f", 1): (8268, 9970), ("d", 0): (6889, 7097), ("d", 1): (6835, 7140)}
# (T, robot): phase_leg_rt<UI = false>, <UI = true>, phase_front_team (both UI), phase_base_lead, phase_finish_team, phase_integrate_team
PARENT_PHASES = {("f", 0): (1345, 1379, 1632, 346, 468, 253), ("f", 1): (1958, 1998, 1986, 346, 468, 254),
                 ("d", 0): (1619, 1657, 1881, 398, 564, 488), ("d", 1): (2349, 2386, 2286, 398, 564, 488)}
# Workgroup barriers (s_barrier) as instructions.  The kernel body holds four: the main wavefront's barrier A (substep_team), the
# helper's A and B (substep_team_helper), and the one behind the SOLORL_POISON_LDS fill; the main wavefront's barrier B is the one
# in each phase_leg_rt<DUO = true> instantiation.  Executed per step and role: 2 x frame_skip (+ 1 with the poison hook on).
BARRIERS_IN_KERNEL, BARRIERS_IN_LEG_PHASE = 4, 1


@pytest.fixture(scope="module")
def code():
    from solorl_amd import devcode
    build.build()
    return devcode.function_stats(build.LIB), devcode.kernel_resources(build.LIB), devcode.kernel_static_lds(build.LIB)


def _one(stats, pattern):
    hits = [n for n in stats if re.search(pattern, n)]
    assert len(hits) == 1, (pattern, hits)
    return hits[0]


@pytest.mark.parametrize("robot", [0, 1])
def test_duo_kernels_exist_within_the_step_kernels_bounds(code, robot):
    stats, res, lds = code
    duo = _one(res, r"duo_kernel_teamIfLi%dEEE" % robot)
    classic = _one(res, r"16step_kernel_teamIfLi%dEEE" % robot)
    assert "step_kernel" not in duo
    assert lds[duo] == 0 and res[duo]["group_segment_fixed_size"] == 0
    assert res[duo]["vgpr_count"] <= 256 and res[duo]["agpr_count"] == 0, res[duo]
    assert res[duo]["private_segment_fixed_size"] <= res[classic]["private_segment_fixed_size"], (res[duo], res[classic])
    assert res[duo]["max_flat_workgroup_size"] == 128 and res[classic]["max_flat_workgroup_size"] == 64
    assert not [n for n in res if "duo_kernel_teamId" in n]          # fp32 only


@pytest.mark.parametrize("robot", [0, 1])
def test_duo_barrier_count(code, robot):
    stats, _, _ = code
    assert stats[_one(stats, r"duo_kernel_teamIfLi%dEEE" % robot)]["barriers"] == BARRIERS_IN_KERNEL
    legs = [n for n in stats if re.search(r"phase_leg_rtIfLi%dE.*Lb[01]ELb1EEE" % robot, n)]
    assert len(legs) == 2, legs                                      # UI = false / true
    for n in legs:
        assert stats[n]["barriers"] == BARRIERS_IN_LEG_PHASE, (n, stats[n])
    fronts = [n for n in stats if re.search(r"phase_front_teamIfLi%dE.*Lb[01]ELb1EEE" % robot, n)]
    assert len(fronts) == 2 and all(stats[n]["barriers"] == 0 for n in fronts)
    # nothing else in the engine's step code holds one: the classic kernels and every other phase run one wavefront per workgroup
    for n, s in stats.items():
        if re.search(r"solo\d+phase_|pgs_team|step_kernel|rollout_kernel", n) and not re.search(r"phase_leg_rtIf.*Lb[01]ELb1EEE", n):
            assert s["barriers"] == 0, n


@pytest.mark.parametrize("T,robot", sorted(PARENT_KERNELS))
def test_classic_kernels_and_phases_are_the_parents_code(code, T, robot):
    stats, _, _ = code
    step, roll = PARENT_KERNELS[(T, robot)]
    leg0, leg1, front, lead, finish, integ = PARENT_PHASES[(T, robot)]
    tr = "I%sLi%dE" % (T, robot)
    want = {r"16step_kernel_team%sEE" % tr: step, r"rollout_kernel_team%sEE" % tr: roll,
            r"phase_leg_rt%s.*CtxLds.*EEELb0ELb0EEE" % tr: leg0, r"phase_leg_rt%s.*CtxLds.*EEELb1ELb0EEE" % tr: leg1,
            r"phase_front_team%s.*EEELb0ELb0EEE" % tr: front, r"phase_front_team%s.*EEELb1ELb0EEE" % tr: front,
            r"phase_base_lead%s" % tr: lead, r"phase_finish_team%s" % tr: finish, r"phase_integrate_team%s" % tr: integ}
    for pattern, n in want.items():
        name = _one(stats, pattern)
        print(name[:100], stats[name]["body"], "parent", n)
        assert stats[name]["body"] == n, (name, stats[name], n)


def test_duo_phases_add_only_the_barrier(code):
    """the helper's front is the classic one minus the C.R0 store, the main wavefront's leg phase the classic one plus barrier B
    (fences and waits around it: a handful of instructions, no spill -- __syncthreads() as a call cost 280 and two scratch slots)"""
    stats, _, _ = code
    for robot in (0, 1):
        for ui in (0, 1):
            leg_c = stats[_one(stats, r"phase_leg_rtIfLi%dE.*EEELb%dELb0EEE" % (robot, ui))]
            leg_d = stats[_one(stats, r"phase_leg_rtIfLi%dE.*EEELb%dELb1EEE" % (robot, ui))]
            assert 0 < leg_d["body"] - leg_c["body"] <= 16 and leg_d["scratch"] == 0, (leg_c, leg_d)
            fr_c = stats[_one(stats, r"phase_front_teamIfLi%dE.*EEELb%dELb0EEE" % (robot, ui))]
            fr_d = stats[_one(stats, r"phase_front_teamIfLi%dE.*EEELb%dELb1EEE" % (robot, ui))]
            assert fr_d["body"] <= fr_c["body"] and fr_d["scratch"] <= fr_c["scratch"], (fr_c, fr_d)
