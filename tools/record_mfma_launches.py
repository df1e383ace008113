#!/usr/bin/env python3
"""Record what every case of tests/mfma_plan_cases.py launches: the last_row_kernel / last_hess_kernel / last_dense_writer
codes after the call and, from a `rocprofv3 --kernel-trace` of the run, the name, grid size (workgroups) and workgroup size of
each library kernel the call launched.

    tools/record_mfma_launches.py [--out tests/golden/mfma_launches.json] [--lds-out FILE] [--dir build/mfma_launches]

NEMPC_LIB selects the library (the parent's build before a change of the dispatch, the branch's after it).  --lds-out also
writes the LDS bytes the trace reports per launch (compared trace against trace; not part of the golden file).

The worker (--worker) runs the cases in one process; a case's call sits between two launches of a sentinel (a torch
bitwise-xor kernel nothing else in the run uses), which is how the trace is cut into cases."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

SENTINEL = "xor"


def worker(codes_path):
    import torch
    import mfma_plan_cases as mc
    sent = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    codes = {}
    for case in mc.CASES:
        # the engine is created (and its first call's buffers allocated) before the opening sentinel: a warm-up call
        # would launch the same kernels twice, so the sentinel goes in by wrapping the library call itself
        import pyneuralempc_amd._lib as _lib
        lib = _lib.load()
        wrapped = {}
        for fn in ("nempc_eval", "nempc_hess", "nempc_hess_gn"):
            real = getattr(lib, fn)
            wrapped[fn] = real

            def call(*a, _real=real):
                torch.cuda.synchronize()
                torch.bitwise_xor(sent, sent, out=sent)
                rc = _real(*a)
                torch.bitwise_xor(sent, sent, out=sent)
                torch.cuda.synchronize()
                return rc
            setattr(lib, fn, call)
        try:
            codes[case["id"]], _, eng = mc.run(case)
        finally:
            for fn, real in wrapped.items():
                setattr(lib, fn, real)
        del eng
    with open(codes_path, "w") as fh:
        json.dump(codes, fh)


def cut_trace(path):
    """-> one list of launches per pair of sentinels, in dispatch order"""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cases, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if SENTINEL in name.lower() and "nempc" not in name:
            if cur is None:
                cur = []
            else:
                cases.append(cur)
                cur = None
        elif cur is not None and "nempc" in name:
            wg = int(r["Workgroup_Size_X"])
            cur.append(dict(name=name, grid=int(r["Grid_Size_X"]) // wg, wg=wg, lds=int(r.get("LDS_Block_Size") or r["Group_Segment_Size"])))
    assert cur is None, "odd number of sentinels in the trace"
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "mfma_launches.json"))
    ap.add_argument("--lds-out")
    ap.add_argument("--dir", default=os.path.join(REPO, "build", "mfma_launches"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    import mfma_plan_cases as mc
    os.makedirs(a.dir, exist_ok=True)
    codes_path = os.path.join(a.dir, "codes.json")
    env = dict(os.environ, TMPDIR="/tmp")
    with open(os.path.join(a.dir, "worker.log"), "w") as log:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(a.dir, "trace"), "--",
                        sys.executable, os.path.abspath(__file__), "--worker", codes_path], check=True, cwd=REPO, env=env,
                       stdout=log, stderr=subprocess.STDOUT)
    traces = glob.glob(os.path.join(a.dir, "trace", "**", "*kernel_trace.csv"), recursive=True)
    assert len(traces) == 1, traces
    cuts = cut_trace(traces[0])
    codes = json.load(open(codes_path))
    assert len(cuts) == len(mc.CASES), (len(cuts), len(mc.CASES))
    golden, lds = {}, {}
    for case, launches in zip(mc.CASES, cuts):
        golden[case["id"]] = dict(codes[case["id"]], launches=[{k: l[k] for k in ("name", "grid", "wg")} for l in launches])
        lds[case["id"]] = [l["lds"] for l in launches]
    with open(a.out, "w") as fh:
        json.dump(golden, fh, indent=0, sort_keys=True)
        fh.write("\n")
    if a.lds_out:
        with open(a.lds_out, "w") as fh:
            json.dump(lds, fh, indent=0, sort_keys=True)
    print(f"{len(golden)} cases -> {a.out}")


if __name__ == "__main__":
    main()
