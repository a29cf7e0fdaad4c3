"""Bit pins of solorl_kinematics and solorl_dynamics (tests/test_rows_bits_gpu.py): sha256 of every output row of both calls.

    python tests/golden/make_golden_rows_bits.py            # writes tests/golden/rows_bits.json (needs the GPU)
    python tests/golden/make_golden_rows_bits.py --check    # runs every case twice and compares, writes nothing

The committed fixture was generated on an MI355X with the library of commit 1da4216 ("Duo step kernel: base pose and next R0 on the
helper behind barrier D"), i.e. BEFORE the two kernels' shells were folded into csrc/row_batch.hpp: that change, and any later one
that is meant to leave the arithmetic alone, has to reproduce these hashes.  Regenerate only after a compiler change, with the
then-current parent -- never with the code under test.

Inputs come from numpy alone (tests/kin_util.random_states under a fixed seed per case), so they are the same on every machine.
Per (query, robot, urdf): n = 1; n = 59 (four workgroups of either kernel, the last ragged: 18 * 3 + 5 and 16 * 3 + 11); and n = 59
under a mask (i % 3 != 1, rows 16..35 all off so that one workgroup of either kernel has nothing live) into an `out` pre-filled with
byte 0xA5, the masked input rows set to NaN -- all 59 rows are hashed, the untouched ones included.  Per launch: the first 16 hex
digits of the sha256 of each row's bytes (enough to locate a difference) and the sha256 of the whole buffer."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "rows_bits.json")
N = 59
QUERIES = ("kinematics", "dynamics")
CASES = [(robot, urdf) for robot in (0, 1) for urdf in (0, 1)]


def case_name(query, robot, urdf):
    return "%s_%s_%s" % (query, "solo12" if robot else "solo8", "urdf" if urdf else "box")


def mask_rows():
    m = np.arange(N) % 3 != 1
    m[16:36] = False
    return m


def _hashes(buf):
    """buf: uint8 [n, row bytes] (numpy)"""
    return {"rows": [hashlib.sha256(r.tobytes()).hexdigest()[:16] for r in buf], "all": hashlib.sha256(buf.tobytes()).hexdigest()}


def run_case(query, robot, urdf):
    """{launch: {"rows": [...], "all": ...}} of the three launches of one case"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch
    from solorl_amd import dyn_tensors as D, kinematics as K
    from solorl_amd.state import StateBatch
    from tests import kin_util as ku
    call, batch, row_bytes = (K.kinematics, K.KinBatch, K.ROW_BYTES) if query == "kinematics" else (D.dynamics, D.DynBatch, D.ROW_BYTES)
    cfg = ku.kin_cfg(robot, urdf)
    dev = torch.device("cuda:0")
    states = StateBatch.from_env_states(ku.random_states(cfg, N, np.random.default_rng(7100 + 10 * robot + urdf)), dev)
    out = {}
    out["n1"] = _hashes(call(cfg, StateBatch(data=states.data[:1].clone())).bytes().cpu().numpy())
    out["n59"] = _hashes(call(cfg, states).bytes().cpu().numpy())
    mask = torch.from_numpy(mask_rows()).to(dev)
    holed = states.clone()
    holed.data[~mask] = float("nan")
    dst = batch(data=torch.full((N, row_bytes), 0xA5, dtype=torch.uint8, device=dev).view(torch.float64))
    out["n59_masked"] = _hashes(call(cfg, holed, mask=mask, out=dst).bytes().cpu().numpy())
    torch.cuda.synchronize()
    return out


def run_all():
    return {case_name(q, r, u): run_case(q, r, u) for q in QUERIES for r, u in CASES}


def main():
    a = run_all()
    if "--check" in sys.argv:
        b = run_all()
        print(json.dumps({k: {l: v[l]["all"] for l in v} for k, v in a.items()}, indent=1))
        print("two runs agree" if a == b else "TWO RUNS DIFFER")
        return 0 if a == b else 1
    with open(FIXTURE, "w") as f:
        json.dump(a, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)
    return 0


if __name__ == "__main__":
    sys.exit(main())
