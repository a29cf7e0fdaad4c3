"""solorl_amd/build.py's flag record: objects of a build that failed or was interrupted are never linked by a later build under other
flags.  A stub stands in for hipcc (it writes its command line where the object would go); the real library is not touched."""
import os
import subprocess
import sys

import pytest

from solorl_amd import build

STUB = """#!%s
import os, sys
a = sys.argv[1:]
open(a[a.index("-o") + 1], "w").write(" ".join(a))
sys.exit(1 if "-DSOLO_TU_PART=" + os.environ.get("STUB_FAIL_PART", "none") in a else 0)
"""


def test_failed_build_leaves_no_flag_record(tmp_path, monkeypatch):
    obj = tmp_path / "obj"
    monkeypatch.setattr(build, "OBJ", str(obj))
    monkeypatch.setattr(build, "LIB", str(tmp_path / "libsolorl_hip.so"))
    monkeypatch.setattr(build, "TAG", str(obj / "flags.txt"))
    stub = tmp_path / "hipcc_stub"
    stub.write_text(STUB % sys.executable)
    stub.chmod(0o755)
    monkeypatch.setenv("HIPCC", str(stub))
    monkeypatch.delenv("SOLORL_BUILD_DEFINES", raising=False)
    monkeypatch.delenv("SOLORL_BUILD_FLAGS", raising=False)
    monkeypatch.delenv("STUB_FAIL_PART", raising=False)

    def objects():
        return {f: (obj / f).read_text() for f in sorted(os.listdir(obj)) if f.endswith(".o")}

    # a plain build: record written, nothing to do afterwards
    assert build.needs_build()
    build.build()
    assert os.path.exists(build.TAG) and os.path.exists(build.LIB) and not build.needs_build()
    assert len(objects()) == 7 and not any("SOLO_MARK" in c for c in objects().values())        # five engine parts, PPO, normalisation

    # a build under other flags in which one part fails: the other parts' objects now carry the new flags ...
    monkeypatch.setenv("SOLORL_BUILD_DEFINES", "SOLO_MARK")
    monkeypatch.setenv("STUB_FAIL_PART", "2")
    assert build.needs_build()
    with pytest.raises(subprocess.CalledProcessError):
        build.build()
    assert sum("-DSOLO_MARK" in c for c in objects().values()) >= 6
    # ... and no record says which: the plain flags need a build again, and it compiles every part
    assert not os.path.exists(build.TAG)
    monkeypatch.delenv("SOLORL_BUILD_DEFINES")
    monkeypatch.delenv("STUB_FAIL_PART")
    assert build.needs_build()
    build.build()
    assert os.path.exists(build.TAG) and not build.needs_build()
    assert len(objects()) == 7 and not any("SOLO_MARK" in c for c in objects().values())
