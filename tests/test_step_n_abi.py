"""K-step launches (include/solorl.h solorl_step_n, solorl_rollout) without a GPU: the entry points follow the error convention, and the
built code object has the four K-step kernels with no static LDS and no more registers or scratch than the one-step team kernel of the
same arithmetic type and robot."""
import ctypes as C
import re

import pytest

from solorl_amd import _native, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_step_n_and_rollout_reject_a_null_handle_and_k0(lib):
    assert lib.solorl_step_n(None, 1, None, None, None, None, None, None) == -1
    assert b"null handle" in lib.solorl_last_error()
    assert lib.solorl_step_n(None, 0, None, None, None, None, None, None) == -1
    assert b"K must be >= 1" in lib.solorl_last_error()
    P = _native.PolicyParams()
    P.obs_dim, P.act_dim, P.hidden = 76, 12, 64
    assert lib.solorl_rollout(None, 4, None, None, None, None, None, C.byref(P), None, None, None, 1, None) == -1
    assert b"null handle" in lib.solorl_last_error()
    assert lib.solorl_rollout(None, 0, None, None, None, None, None, C.byref(P), None, None, None, 0, None) == -1
    assert b"K must be >= 1" in lib.solorl_last_error()


def _kernels(name_part):
    from solorl_amd import devcode
    res = devcode.kernel_resources(build.LIB)
    out = {}
    for k, v in res.items():
        m = re.search(name_part + r"I([fd])Li([01])E", k)
        if m:
            out[(m.group(1), int(m.group(2)))] = v
    return out


def test_k_step_kernels_have_no_static_lds_and_the_step_kernels_registers(lib):
    """rollout_kernel_team<T, ROBOT> runs step_team in a loop: the loop must not keep the launch's arguments in registers across the
    steps (read as kernel parameters they were hoisted out of it: 150 spilled VGPRs and twice the scratch).  Margins: 8 registers of
    each kind, 64 B of scratch per lane (the loop counter, the argument pointer, the step's row offsets)."""
    from solorl_amd import devcode
    lds = {k: v for k, v in devcode.kernel_static_lds(build.LIB).items() if "rollout_kernel_team" in k}
    assert len(lds) == 4, sorted(lds)            # {fp32, fp64} x {Solo8, Solo12}
    assert all(v == 0 for v in lds.values()), lds
    step, roll = _kernels("16step_kernel_team"), _kernels("19rollout_kernel_team")
    assert sorted(step) == sorted(roll) == [("d", 0), ("d", 1), ("f", 0), ("f", 1)], (sorted(step), sorted(roll))
    for key in step:
        s, r = step[key], roll[key]
        assert r["group_segment_fixed_size"] == 0, (key, r)
        assert r["vgpr_count"] <= s["vgpr_count"] + 8 and r["agpr_count"] <= s["agpr_count"] + 8, (key, s, r)
        if key[0] == "f":                  # (the fp32 kernel is the product path: its spills stay where the step kernel's are)
            assert r.get("vgpr_spill_count", 0) <= s.get("vgpr_spill_count", 0) + 8, (key, s, r)
        assert r["private_segment_fixed_size"] <= s["private_segment_fixed_size"] + 64, (key, s, r)
