"""strata_stats.json in $SOLORL_STATS_DIR or build/strata (written by tests/test_strata_cpu.py and the -m gpu cases of tests/test_strata_gpu.py through
tests/strata_util.py record) -> tests/golden/strata_measured.json: the host build's fp32 figures per stratum (host/), the oracle twins'
(oracle/), and the rho quantiles MEASURED on the MI355X in mode f32-team-helper on the calibration strata (gpu/calibration), which every
fp32 mode's strata are then held to within PARITY_MARGIN (3 x).  Sections the run did not produce keep what the file had.  Run after
a test run whose numbers are to become the reference; prints the calibration."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.environ.get("SOLORL_STATS_DIR") or os.path.join(ROOT, "build", "strata"), "strata_stats.json")
new = json.load(open(src))
dst = os.path.join(ROOT, "tests", "golden", "strata_measured.json")
cur = json.load(open(dst)) if os.path.exists(dst) else {}
for k in ("host", "oracle"):
    if k in new:
        cur[k] = new[k]
if "calibration" in new.get("gpu", {}):
    cur.setdefault("gpu", {})["calibration"] = new["gpu"]["calibration"]
json.dump(cur, open(dst, "w"), indent=1, sort_keys=True)
for robot, q in sorted(cur.get("gpu", {}).get("calibration", {}).items()):
    print("gpu/calibration/%s: n %d  rho p50 %.3g  p90 %.3g  p99 %.3g" % (robot, q["n"], q["p50"], q["p90"], q["p99"]))
