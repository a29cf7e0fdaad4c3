"""The common path of the K7 team sweeps, from the built gfx950 code object (no GPU needed).

`devcode.loop_stats` counts the whole span of a sweep loop, the cold block that publishes a team's result included
(tests/test_sweep_issue_slots.py); `devcode.hot_path_stats` counts what a sweep issues when no team leaves in it -- all but four of a
solve's sweeps.  The cone sweeps are GATED ("Issue slots per sweep"): their friction
pairs' K7 residual entries are formed in the cold block, only in sweeps in which some unfinished team's limit and normal rows were all
quiet, and no longer in the slots.  Pinned here: the common path without them, and a cold block that still computes all of them."""
import collections
import os
import re

import pytest

from solorl_amd import build

# common path of pgs_team_variant<float, RowLds<float,4>, LIM, 4, 8, true, true, true>: at most the count of the scratch-copy prototype
# this change was planned on (303 with the limit slot, 281 without) plus 1 %; the parent d6e7947 issues 324 / 302 (same counting function)
MAX_HOT = {(1, 4, 8, 1): 306, (0, 4, 8, 1): 284}
PARENT_HOT = {(1, 4, 8, 1): 324, (0, 4, 8, 1): 302}

def gate_min_nfs():
    """fewest friction slots of a gated cone sweep: the default of SOLO_K7_GATE_MIN_NFS in the kernel source"""
    src = open(os.path.join(os.path.dirname(build.SRC[1]), "dynamics.hpp")).read()
    return int(re.search(r"^#define SOLO_K7_GATE_MIN_NFS (\d+)", src, re.M).group(1))


@pytest.fixture(scope="module")
def sweeps():
    from solorl_amd import devcode
    build.build()
    text = devcode.disassemble(build.LIB)
    loops = devcode.loop_stats(build.LIB, "pgs_team_variantIfNS", text=text)
    hot = devcode.hot_path_stats(build.LIB, "pgs_team_variantIfNS", text=text)
    out = {}
    for n, s in loops.items():
        m = re.search(r"Li(\d)ELi(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)EEE", n)
        lim, nn, nf, early, pipe, cone = (int(x) for x in m.groups())
        if early and nn + nf > 0:
            span = collections.Counter(s["ops_in_loop"])
            out[(lim, nn, nf, cone)] = dict(loop=s, hot=hot[n], hot_ops=collections.Counter(hot[n]["ops"]), span_ops=span)
    return out


def test_all_k7_sweeps_found(sweeps):
    assert len(sweeps) == 32                         # {limit slot or not} x {1..8 contacts} x {pyramid, cone}
    for key, s in sweeps.items():
        assert s["hot"]["head"] is not None and 0 < s["hot"]["insts"] < s["loop"]["insts_in_loop"], (key, s["hot"]["insts"])


@pytest.mark.parametrize("key", sorted(MAX_HOT))
def test_common_path_of_the_heaviest_cone_sweeps(sweeps, key):
    s = sweeps[key]
    nfs = key[2]
    print(key, "common path %d instructions (%d s_nop, %d K7-only), parent %d; loop span %d" %
          (s["hot"]["insts"], s["hot"]["s_nop"], s["hot"]["k7_only"], PARENT_HOT[key], s["loop"]["insts_in_loop"]))
    assert s["hot"]["insts"] <= MAX_HOT[key]
    assert s["hot_ops"]["v_max3_f32"] == 0                        # the pairs' running maximum is off the common path
    assert s["hot_ops"]["v_mul_f32_e32"] == nfs                   # one multiply per cone slot (the new impulse), not two
    # the cold block forms every pair's entry: as many v_max3_f32 (one per two slots) and v_rsq_f32 in the span as before
    assert s["span_ops"]["v_max3_f32"] == nfs // 2 == 4
    assert s["span_ops"]["v_rsq_f32_e32"] == nfs == 8


def test_gated_sweeps_keep_the_pairs_entries_in_the_cold_block(sweeps):
    gated = 0
    for (lim, nn, nf, cone), s in sorted(sweeps.items()):
        if cone and nf >= gate_min_nfs():
            gated += 1
            assert s["hot_ops"]["v_max3_f32"] == 0 and s["hot_ops"]["v_mul_f32_e32"] == nf, (lim, nn, nf)
            # (the parent's counts: one v_max3_f32 per two slots -- an odd last slot takes a v_max_f32 -- and one v_rsq_f32 per slot)
            assert s["span_ops"]["v_max3_f32"] == nf // 2 and s["span_ops"]["v_rsq_f32_e32"] == nf, (lim, nn, nf)
    assert gated >= 8                                # (five friction slots or more, with and without the limit slot, at the least)


def test_no_memory_access_in_any_k7_sweep_loop(sweeps):
    for key, s in sorted(sweeps.items()):
        assert s["loop"]["scratch_in_loop"] == 0 and s["loop"]["lds_reads_in_loop"] == 0 and s["loop"]["vmem_in_loop"] == 0, (key, s["loop"])
