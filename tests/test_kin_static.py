"""Static checks of solorl_kinematics (no GPU): the built kernels use no scratch and two workgroups of them fit a CU by registers and by LDS (read from
the code object's metadata, as tests/test_abi.py does for the step kernels), the Python mirror of solorl_env_kin agrees with the
header, and the arguments the entry point must refuse are refused before any HIP call."""
import re

import pytest

from solorl_amd import _native, build
from solorl_amd.config import default_config, ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK
from solorl_amd import kinematics as K
from solorl_amd.state import ROW_BYTES as STATE_ROW_BYTES
from tests import rows_util as ru


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_kernels_use_no_scratch_and_two_workgroups_fit_a_cu(lib):
    """Residency from BOTH limits, as the hardware counts them (tests/rows_util.residency, which also holds the kernels and sincos_call
    to no scratch and no FLAT access)."""
    envs, kernels = ru.residency("kin")
    assert envs == K.ENVS_PER_WORKGROUP
    for name, r, lds, by_regs, by_lds in kernels:
        assert lds == envs * (74 + K.ROW_WORDS) * 8 + envs * 4, (name, r)   # staged rows in and out plus the rows' live flags
        assert min(by_regs, by_lds) == 2, (name, r, lds, by_regs, by_lds)       # what DESIGN.md and the kernel's comment say


def test_python_mirror_matches_the_header():
    hdr, dims, declared = ru.declared_members("solorl_env_kin", ("SOLORL_KIN_MAX_LINKS", "SOLORL_STATE_MAX_PRIMS"))
    assert declared == [(n, K.MEMBERS[n][1]) for n, _ in K.EnvKin._fields_]
    assert K.ROW_BYTES == 3640 and STATE_ROW_BYTES == 2040 and K.KIN_MAX_LINKS == dims["SOLORL_KIN_MAX_LINKS"]
    assert len(K.LINK_NAMES[ROBOT_SOLO8]) == 13 and len(K.LINK_NAMES[ROBOT_SOLO12]) == 17
    assert K.LINK_NAMES[ROBOT_SOLO12][0] == "base_link" and K.LINK_NAMES[ROBOT_SOLO12][4] == "FL_FOOT"
    assert re.search(r"#define SOLORL_ABI_VERSION 5\b", hdr)             # no existing struct changed


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """null cfg / states / out, n < 1, a bad robot, sim_dt <= 0: SOLORL_ERR_INVALID, the message names the function -- on a machine
    without a GPU too, so the check precedes the first HIP call (which would answer SOLORL_ERR_NODEVICE there)"""
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    bad_robot = cfg.copy(); bad_robot.robot = 2
    bad_dt = cfg.copy(); bad_dt.sim_dt = 0.0
    neg_dt = cfg.copy(); neg_dt.sim_dt = -1.0 / 240
    nan_dt = cfg.copy(); nan_dt.sim_dt = float("nan")
    ru.assert_refused("solorl_kinematics", cfg, [bad_robot, bad_dt, neg_dt, nan_dt])
