// What csrc/mfma_plan.h (plain host code) plans for the calls of the input-gather sweep: tests/test_input_gather_cases_cpu.py
// builds this, feeds it one line per (case, compute units) and compares the answers with the Python restatement in
// tests/input_gather_cases.py.
//   input_gather_plan_check QUERIES
//   line in:  id esz wp nh nx nu nin ne window integrator variant act n m B H num_cus
//   line out: id num_cus tiles dense defect hess tpw per_cu rows_resident hess_resident passes
// tiles / dense / defect: RowKernel of an evaluation asking for tiles + dense + band values, for the dense matrix alone (16-byte
// aligned), for the defects alone; hess: HessKernel of the tril values (inside the RK4 pipeline: of its direct-mode launch);
// tpw, per_cu, passes: the cooperative row kernel's tiles per pass, workgroups per compute unit and most passes of a workgroup
// (0 where the rows are not its).
#include <cstdio>

#include "mfma_plan.h"

using namespace nempc;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* fh = std::fopen(argv[1], "r");
    if (!fh) { std::printf("cannot open %s\n", argv[1]); return 2; }
    char id[128];
    const MfmaKnobs kn;
    while (std::fscanf(fh, "%127s", id) == 1) {
        MfmaShape s{};
        if (std::fscanf(fh, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &s.esz, &s.wp, &s.nh, &s.nx, &s.nu, &s.nin, &s.ne, &s.window,
                        &s.integrator, &s.variant, &s.act, &s.n, &s.m, &s.B, &s.H, &s.num_cus) != 16) {
            std::printf("bad line for %s\n", id);
            return 2;
        }
        s.obj_elems = 4 * s.nx * s.nx + 2 * s.nu * s.nu + 2 * s.H * (s.nx + s.nu);     // (every handle holds an objective table)
        s.hess_scatter = s.window == 1; s.layered_hess = false;
        RowsWant w;
        w.bits = WANT_TILES | WANT_DENSE | WANT_SPARSE;
        const MfmaRowsPlan tiles = plan_rows(s, w, kn);
        w.bits = WANT_TILES;
        const MfmaRowsPlan only_tiles = plan_rows(s, w, kn);
        w.bits = WANT_TILES | WANT_GN;
        const MfmaRowsPlan gn = plan_rows(s, w, kn);
        if (only_tiles.kernel != tiles.kernel || gn.kernel != tiles.kernel || gn.covers || only_tiles.tpw != tiles.tpw) {
            std::printf("%s: the tile requests disagree: %d %d %d\n", id, tiles.kernel, only_tiles.kernel, gn.kernel);
            return 1;
        }
        w.bits = WANT_TILES | WANT_DENSE;
        const MfmaRowsPlan dense = plan_rows(s, w, kn);
        if (dense.family == FAM_COOP && (dense.tpw != tiles.tpw || dense.g.per_cu != tiles.g.per_cu)) {
            std::printf("%s: the dense request has its own pass size\n", id);
            return 1;
        }
        w.bits = 0;
        const MfmaRowsPlan defect = plan_rows(s, w, kn);
        HessWant hw;
        const bool rk4 = s.integrator == NEMPC_RK4;
        hw.bits = rk4 ? (HWANT_BLOCKS | HWANT_DIRECT) : HWANT_HVALS;
        hw.vdiv = rk4 ? 4 : 1;
        const MfmaHessPlan hess = plan_hess(s, hw, kn);
        const bool coop = tiles.family == FAM_COOP;
        const int per_wg = tiles.g.tiles_per_wg + (tiles.g.tiles_rem ? 1 : 0);
        std::printf("%s %d %d %d %d %d %d %d %d %d %d\n", id, s.num_cus, tiles.kernel, dense.kernel, defect.kernel, hess.kernel,
                    coop ? tiles.tpw : 0, coop ? tiles.g.per_cu : 0, tiles.family == FAM_TILE && tiles.resident ? 1 : 0,
                    hess.family == FAM_TILE && hess.resident ? 1 : 0, coop ? (per_wg + tiles.tpw - 1) / tiles.tpw : 0);
    }
    std::fclose(fh);
    return 0;
}
