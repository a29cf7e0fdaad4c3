"""Batched state access (include/solorl.h solorl_get_states, solorl_set_states, solorl_reset_masked) without a GPU: the entry points
follow the error convention, the built code object holds the two copy kernels for both arithmetic types without scratch, and
StateBatch's views sit where the ctypes EnvState puts the members."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from solorl_amd import _native, build
from solorl_amd.config import EnvState, ABI_VERSION
from solorl_amd.state import StateBatch, MEMBERS, ROW_BYTES, ROW_WORDS, field_bits, FIELD_BITS, GROUP_MEMBERS


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_batched_state_entry_points_reject_a_null_handle(lib):
    assert lib.solorl_get_states(None, None, None, None) == -1
    assert b"solorl_get_states" in lib.solorl_last_error()
    assert lib.solorl_set_states(None, None, None, 255, None) == -1
    assert b"solorl_set_states" in lib.solorl_last_error()
    assert lib.solorl_reset_masked(None, None, None, None) == -1
    assert b"solorl_reset_masked" in lib.solorl_last_error()


def test_abi_version_is_unchanged(lib):
    assert lib.solorl_abi_version() == 5 == ABI_VERSION


def test_copy_kernels_exist_for_both_types_and_use_no_scratch(lib):
    """A copy kernel has no reason to touch scratch: the row-word table is read from device memory (indexed by lane as a kernel
    argument it would be copied to private memory)."""
    from solorl_amd import devcode
    res = devcode.kernel_resources(build.LIB)
    for kern in ("get_states_kernel", "set_states_kernel"):
        found = {}
        for k, v in res.items():
            m = re.search(r"\d+" + kern + r"I([fd])E", k)
            if m:
                found[m.group(1)] = v
        assert sorted(found) == ["d", "f"], (kern, sorted(res))
        for t, r in found.items():
            assert r["private_segment_fixed_size"] == 0, (kern, t, r)
            assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (kern, t, r)


def test_state_batch_views_agree_with_the_ctypes_struct():
    """A distinct value written through every view is read back from env_state(i) under the same member name, and every
    byte of a row is covered by exactly one view."""
    assert ROW_BYTES == C.sizeof(EnvState) and ROW_WORDS * 8 == ROW_BYTES
    N = 3
    sb = StateBatch(N, "cpu")
    assert sb.data.shape == (N, ROW_WORDS) and sb.data.dtype == torch.float64
    expected_shapes = dict(pos=(N, 3), quat=(N, 4), lin_vel=(N, 3), ang_vel=(N, 3), q=(N, 12), qd=(N, 12), tau=(N, 12), lambda_prev=(N, 24),
                           hist=(N, 4, 42), goal=(N, 2), potential=(N,), progress=(N,), goals_reached=(N,), env_goals_reached=(N,),
                           dr=(N, 5), treadmill_y=(N,), timestep=(N,), need_reset=(N,), contact_mask=(N,), rng_counter=(N,))
    assert sorted(expected_shapes) == sorted(n for n, _ in EnvState._fields_) == sorted(MEMBERS)
    base = 1000
    for name, shape in expected_shapes.items():
        v = getattr(sb, name)
        assert tuple(v.shape) == shape, name
        is_int = name in ("timestep", "need_reset", "contact_mask", "rng_counter")
        assert v.dtype == (torch.int32 if is_int else torch.float64), name
        n = int(np.prod(shape))
        v.copy_(torch.arange(base, base + n, dtype=v.dtype).reshape(shape))
        base += n
    assert base - 1000 == N * (ROW_BYTES - 16) // 8 + N * 4          # every member element got its own value
    base = 1000
    for name, shape in expected_shapes.items():
        per_env = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        for i in range(N):
            got = np.asarray(getattr(sb.env_state(i), name), dtype=np.float64).reshape(-1)
            want = np.arange(base + i * per_env, base + (i + 1) * per_env, dtype=np.float64)
            assert np.array_equal(got, want), (name, i, got, want)
        base += N * per_env
    # offsets as such
    for name, (off, shape, is_int) in MEMBERS.items():
        assert off == getattr(EnvState, name).offset
    c = sb.clone()
    assert torch.equal(c.data, sb.data) and c.data.data_ptr() != sb.data.data_ptr()


def test_state_batch_from_env_states_round_trips_bytes():
    rng = np.random.default_rng(5)
    rows = []
    for i in range(4):
        raw = rng.integers(0, 256, size=ROW_BYTES, dtype=np.uint8).tobytes()      # arbitrary bit patterns, NaNs among them
        rows.append(EnvState.from_buffer_copy(raw))
    sb = StateBatch.from_env_states(rows, "cpu")
    assert sb.num_envs == 4
    for i, s in enumerate(rows):
        assert bytes(sb.env_state(i)) == bytes(s)
        assert sb.bytes()[i].numpy().tobytes() == bytes(s)


def test_field_names():
    assert field_bits("all") == 255 and field_bits(("pose", "vel")) == 3 and field_bits(64) == 64 and field_bits("counters") == 128
    with pytest.raises(ValueError):
        field_bits("velocity")
    assert sorted(GROUP_MEMBERS) == sorted(k for k in FIELD_BITS if k != "all")
    members = sorted(m for g in GROUP_MEMBERS.values() for m in g)
    assert members == sorted(n for n, _ in EnvState._fields_ if n != "tau")
