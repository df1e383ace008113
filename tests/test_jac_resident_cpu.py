"""CPU: nempc_jac_dense_resident is exported and validates its handle, the ABI version is still 8 everywhere, and the table
behind it (csrc/jac_resident.h, plain host code) passes its stand-alone check under the address and undefined-behaviour
sanitizers.  No device call."""
import ctypes
import os
import re
import shutil
import subprocess

from conftest import REPO


def test_export_exists_and_a_null_handle_is_einval():
    from pyneuralempc_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "nempc_jac_dense_resident") and "nempc_jac_dense_resident" in _lib.EXPORTS
    assert lib.nempc_jac_dense_resident(None, None, 0) == _lib.EINVAL
    assert b"nempc_jac_dense_resident" in lib.nempc_last_error()
    assert lib.nempc_jac_dense_resident(None, ctypes.c_void_p(4096), 4) == _lib.EINVAL


def test_abi_version_is_still_8():
    from pyneuralempc_amd import _lib
    text = open(os.path.join(REPO, "include", "nempc.h")).read()
    assert re.search(r"#define NEMPC_ABI_VERSION 8\b", text)
    assert _lib.ABI_VERSION == 8 and _lib.load().nempc_abi_version() == 8
    # the code a full table answers with, in the header and in the binding
    m = re.search(r"#define NEMPC_EFULL \((-\d+)\)", text)
    assert m and int(m.group(1)) == _lib.EFULL
    codes = re.findall(r"#define NEMPC_E[A-Z]+ \((-\d+)\)", text)
    assert len(codes) == len(set(codes))


def test_table_stand_alone_under_sanitizers(tmp_path):
    """tests/jac_resident_check.cpp over csrc/jac_resident.h: lookup, the B limit, capacity, removal, the epoch drop,
    re-registration of a dropped pointer, the epoch's wrap-around."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jac_resident_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "jac_resident_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 60, r.stdout
