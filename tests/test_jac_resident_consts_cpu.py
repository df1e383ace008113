"""CPU: the constants count of the resident dense-Jacobian table (csrc/jac_resident.h, plain host code) passes its stand-alone
check under the address and undefined-behaviour sanitizers.  No device call."""
import os
import re
import shutil
import subprocess

from conftest import REPO


def test_constants_count_stand_alone_under_sanitizers(tmp_path):
    """tests/jac_resident_consts_check.cpp: a fresh registration has no constants, the count follows the evaluated problems up
    to the registered B and never shrinks, a re-registration, a removal and the epoch drop reset it."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jac_resident_consts_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "jac_resident_consts_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 30, r.stdout
