"""The host-only part of koordhip_update_nodes (csrc/snapshot_cols.hpp: the
scatter list over the column table and the staging image), built alone with
the host compiler under AddressSanitizer and UBSan and run as an ordinary
program (tests/snapshot_pack_check.cpp holds the checks)."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _compiler():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


@pytest.mark.skipif(_compiler() is None, reason="needs a host C++ compiler")
def test_snapshot_pack_check_under_sanitizers():
    cxx = _compiler()
    # the sanitizer runtimes linked into the program: it runs as it stands, with nothing to load first
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "snapshot_pack_check")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                        os.path.join(HERE, "snapshot_pack_check.cpp"), "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "snapshot_pack_check ok" in r.stdout
