"""CPU: DevBuf (csrc/dev_buf.h), the type that owns every device allocation of a handle -- the header under sanitizers in a host
program of its own with malloc / free behind its raw functions, what the header may include, and where the library may
spell an allocation."""
import os
import re
import shutil
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, "pyneuralempc_amd", "csrc")


def test_the_buffer_type_passes_the_sanitized_host_program(tmp_path):
    """tests/dev_buf_check.cpp, compiled for the host with AddressSanitizer and UndefinedBehaviorSanitizer and run on its own:
    construction and destruction, a zero-byte allocation's own address, alloc over a held buffer, ensure's grow-only rule, a
    failed allocation, the moves, an array leaving scope, and nempc_set_weights' build-three-then-move-in with each of the
    three allocations failing.  Every case ends with no live allocation."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dev_buf_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, "-I", os.path.join(REPO, "include"), "-o", exe, os.path.join(REPO, "tests", "dev_buf_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-400:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    m = re.search(r"(\d+) cases, (\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) == 8 and int(m.group(2)) >= 60, r.stdout


def test_the_buffer_header_includes_nothing_but_two_standard_headers():
    inc = re.findall(r"^\s*#\s*include\s*(\S+)", open(os.path.join(CSRC, "dev_buf.h")).read(), flags=re.M)
    assert sorted(inc) == ["<cstddef>", "<utility>"]


def test_device_allocations_are_spelled_in_one_unit():
    """hipMalloc( / hipFree( appear in the unit that defines DevBuf's raw functions, and in solver.hip and comm.hip, whose
    workspaces are their own; nowhere else under csrc/."""
    found = sorted(f for f in os.listdir(CSRC)
                   if re.search(r"hipMalloc\(|hipFree\(", open(os.path.join(CSRC, f)).read()))
    definer = [f for f in os.listdir(CSRC)
               if re.search(r"^int dev_raw_alloc\(", open(os.path.join(CSRC, f)).read(), flags=re.M) and not f.endswith(".h")]
    assert definer == ["nempc_api.hip"]
    assert set(found) <= {"nempc_api.hip", "solver.hip", "comm.hip"}, found
    assert "nempc_api.hip" in found
