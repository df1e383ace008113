"""CPU: the host arithmetic of the solver's stage augmentations (csrc/stage_aug.h: stage dimensions, window_var, the window's
index tables, bound slots, the objective table over the augmented stage) without a device -- the header under sanitizers in a
host program of its own, and what it may include."""
import os
import re
import shutil
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, "pyneuralempc_amd", "csrc")


def test_the_augmentation_header_passes_the_sanitized_host_program(tmp_path):
    """tests/stage_aug_check.cpp: csrc/stage_aug.h compiled for the host with AddressSanitizer and UndefinedBehaviorSanitizer and
    run on its own.  H in {1, 2, 5} x nx in {1, 2, 3} x nu in {1, 2} x w in {2, 3, 4} x both window directions (108 cases): the
    window tables against a restatement by labels, dcol against window_var, both objective tables against the caller's
    objective (1e-12 relative; the fp32 table the fp64 one cast element by element), the bound slots."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "stage_aug_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, "-o", exe, os.path.join(REPO, "tests", "stage_aug_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-400:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    m = re.search(r"(\d+) cases, (\d+) entries checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) == 108 and int(m.group(2)) > 100000, r.stdout


def test_the_augmentation_header_includes_nothing_of_hip():
    """stage_aug.h: the C++ library and the two layout headers, which include nothing themselves."""
    inc = re.findall(r"^\s*#\s*include\s*(\S+)", open(os.path.join(CSRC, "stage_aug.h")).read(), flags=re.M)
    assert sorted(inc) == ['"obj_offsets.h"', '"rate_index.h"', "<cstddef>", "<vector>"]
    for name in ("obj_offsets.h", "rate_index.h"):
        assert "#include" not in open(os.path.join(CSRC, name)).read()


def test_the_column_order_and_the_table_layout_have_one_definition():
    """window_var and obj_offsets are defined once (stage_aug.h, obj_offsets.h); the library's units call them."""
    defs = {"window_var": [], "obj_offsets": []}
    for f in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, f)).read()
        for name in defs:
            if re.search(r"^[^\n;=]*\binline\s+\w+\s+%s\(|^\w+\s+%s\(" % (name, name), text, flags=re.M):
                defs[name].append(f)
    assert defs == {"window_var": ["stage_aug.h"], "obj_offsets": ["obj_offsets.h"]}
