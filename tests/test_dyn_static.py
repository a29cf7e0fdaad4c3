"""Static checks of solorl_dynamics (no GPU): the built kernels use no scratch, no AGPRs and no FLAT access, their static LDS is the
staged rows and nothing else, the workgroups per CU that registers and LDS allow are what DESIGN.md states (read from the code object's
metadata, as tests/test_kin_static.py does), the Python mirror of solorl_env_dyn agrees with the header, and the arguments the entry
point must refuse are refused before any HIP call."""
import os
import re

import pytest

from solorl_amd import _native, build
from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
from solorl_amd import dyn_tensors as D
from tests import rows_util as ru


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_kernels_use_no_scratch_no_agprs_and_design_states_their_residency(lib):
    """Residency from BOTH limits, as the hardware counts them (tests/rows_util.residency, which also holds the kernels and sincos_call
    to no scratch and no FLAT access)."""
    envs, kernels = ru.residency("dyn")
    assert envs == D.ENVS_PER_WORKGROUP
    design = open(os.path.join(ru.ROOT, "DESIGN.md")).read()
    stated = int(re.search(r"`dyn_rows_kernel`: (\d+) workgroups? resident per CU", design).group(1))
    assert stated >= 1
    for name, r, lds, by_regs, by_lds in kernels:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r.get("agpr_count", 0) == 0, (name, r)
        assert lds == envs * (37 + D.ROW_WORDS) * 8 + envs * 4, (name, r)   # staged rows in and out plus the rows' live flags
        assert min(by_regs, by_lds) == stated, (name, r, lds, by_regs, by_lds, stated)


def test_python_mirror_matches_the_header():
    hdr, dims, declared = ru.declared_members("solorl_env_dyn", ("SOLORL_DYN_NV",))
    assert declared == [(n, D.MEMBERS[n][1]) for n, _ in D.EnvDyn._fields_]
    assert [n for n, _ in declared] == ["mass_matrix", "bias", "gravity", "foot_jac", "foot_acc_bias", "foot_pos"]
    assert D.ROW_BYTES == 4800 and D.ROW_WORDS == 600 and D.NV == dims["SOLORL_DYN_NV"] == 18
    assert re.search(r"#define SOLORL_ABI_VERSION 5\b", hdr)             # no existing struct changed
    assert re.search(r"^ \*   solorl_dynamics ", hdr, re.M)              # the header's opening list names the entry point


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """null cfg / states / out, n < 1, a bad robot, a non-finite gravity, a non-finite or negative damping: SOLORL_ERR_INVALID, the
    message names the function -- on a machine without a GPU too, so the check precedes the first HIP call (which would answer
    SOLORL_ERR_NODEVICE there)"""
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)

    def with_(**kw):
        c = cfg.copy()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    ru.assert_refused("solorl_dynamics", cfg, [with_(robot=2), with_(robot=-1), with_(gravity=float("nan")), with_(gravity=float("inf")),
                                              with_(damping=float("nan")), with_(damping=float("inf")), with_(damping=-0.04)])
