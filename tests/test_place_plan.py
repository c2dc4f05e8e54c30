"""The place call's decisions (csrc/place_plan.hpp: plan_place, a pure function
of the context's facts and the KOORDHIP_* knobs), built alone with the host
compiler under AddressSanitizer and UBSan and run as an ordinary program
(tests/place_plan_check.cpp holds the hand-worked rows and the grid)."""
import os
import subprocess
import tempfile

import pytest

from test_snapshot_pack import _compiler

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(_compiler() is None, reason="needs a host C++ compiler")
def test_place_plan_check_under_sanitizers():
    cxx = _compiler()
    # the sanitizer runtimes linked into the program: it runs as it stands, with nothing to load first
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "place_plan_check")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                        os.path.join(HERE, "place_plan_check.cpp"), "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "place_plan_check ok" in r.stdout
