"""Barrier C of the helper wavefront (duo_kernel_team, DESIGN section 4 "Helper wavefront") in the built gfx950 code object, no GPU
needed.  The end of the helper's post-B work (leg rates, barrier C: duo_helper_rates) and the main wavefront's join
(duo_join_rows) are two non-inlined device functions, fp32 only; each holds exactly one s_barrier and touches no scratch, and no other
device function gained a barrier -- a mismatched barrier is a hang, so this runs before anything is launched."""
import re

import pytest

from solorl_amd import build

NEW = ("duo_helper_rates", "duo_join_rows")


@pytest.fixture(scope="module")
def code():
    from solorl_amd import devcode
    build.build()
    return devcode.function_stats(build.LIB), devcode.kernel_resources(build.LIB)


def _hits(stats, pattern):
    return [n for n in stats if re.search(pattern, n)]


@pytest.mark.parametrize("robot", [0, 1])
def test_new_functions_exist_for_fp32_only(code, robot):
    stats, res = code
    for fn in NEW:
        hits = _hits(stats, r"solo\d+%sIfLi%dE" % (fn, robot))
        assert len(hits) == 1, (fn, hits)
        assert hits[0] not in res                                    # a device function, not a kernel
        assert not _hits(stats, r"%sId" % fn), fn                    # no fp64 instantiation
    assert len(_hits(stats, "|".join(NEW))) == 2 * len(NEW)          # robots 0 and 1, nothing else by these names


@pytest.mark.parametrize("robot", [0, 1])
def test_one_barrier_each_and_no_scratch(code, robot):
    stats, _ = code
    for fn in NEW:
        s = stats[_hits(stats, r"solo\d+%sIfLi%dE" % (fn, robot))[0]]
        print(fn, robot, s)
        assert s["barriers"] == 1 and s["scratch"] == 0, (fn, s)
    join = stats[_hits(stats, r"solo\d+duo_join_rowsIfLi%dE" % robot)[0]]
    assert join["body"] <= 16 and join["flat"] == 0 and join["global"] == 0, join      # fences, the barrier, the return


def test_no_other_device_function_holds_a_barrier(code):
    """Kernels aside (their barriers are pinned by tests/test_helper_wave_static.py and belong to one-role code), the device
    functions with an s_barrier are exactly: phase_leg_rt<DUO> (B, main), duo_helper_rates (C, helper), duo_join_rows (C, main)."""
    stats, res = code
    holders = sorted(n for n, s in stats.items() if s["barriers"] and n not in res)
    allowed = [n for n in holders if re.search(r"phase_leg_rtIfLi[01]E.*Lb[01]ELb1EEE|solo\d+duo_helper_ratesIfLi[01]E|solo\d+duo_join_rowsIfLi[01]E", n)]
    assert holders == allowed, sorted(set(holders) - set(allowed))
    assert len(holders) == 4 + 2 + 2, holders                        # (robot x UI) leg phases, (robot) helper bases, (robot) joins
    for n, s in stats.items():
        if re.search(r"duo_", n) and n not in res and not re.search("|".join(NEW), n):
            assert s["barriers"] == 0, n


@pytest.mark.parametrize("robot", [0, 1])
def test_duo_kernel_resources(code, robot):
    """<= 256 VGPRs, no AGPRs, scratch no larger than the classic kernel's, with the two new calls in the kernel's call graph"""
    stats, res = code
    duo = [n for n in res if re.search(r"duo_kernel_teamIfLi%dEEE" % robot, n)]
    classic = [n for n in res if re.search(r"16step_kernel_teamIfLi%dEEE" % robot, n)]
    assert len(duo) == 1 and len(classic) == 1
    d, c = res[duo[0]], res[classic[0]]
    assert d["vgpr_count"] <= 256 and d["agpr_count"] == 0, d
    assert d["private_segment_fixed_size"] <= c["private_segment_fixed_size"], (d, c)
