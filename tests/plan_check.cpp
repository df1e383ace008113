// Stand-alone check of csrc/mfma_plan.h (plain host code; tests/test_mfma_plan_cpu.py builds it with the address and
// undefined-behaviour sanitizers and feeds it the recorded launches).
//   plan_check [QUERIES]      QUERIES: one plan query per line with the kernel code, grid and workgroup size recorded on the device
// Prints every enum value with its name, then "<n> checks, <f> failures".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "mfma_plan.h"

using namespace nempc;

static long checks = 0, failures = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        ++checks;                                        \
        if (!(cond)) {                                   \
            ++failures;                                  \
            if (failures < 40) { std::printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                \
    } while (0)

static MfmaShape shape(int esz, int wp, int nh, int nx, int nu, int ne, int integ, int variant, int act, int B, int H, int cus,
                       bool obj = true) {
    MfmaShape s{};
    s.esz = esz; s.wp = wp; s.nh = nh; s.nx = nx; s.nu = nu; s.nin = nx + nu; s.ne = ne; s.window = 1;
    s.integrator = integ; s.variant = variant; s.act = act;
    s.n = H * (nx + nu); s.m = H * nx; s.B = B; s.H = H; s.num_cus = cus;
    s.obj_elems = obj ? 4 * nx * nx + 2 * nu * nu + 2 * H * (nx + nu) : 0;
    s.hess_scatter = true; s.layered_hess = false;
    return s;
}
static RowsWant want(unsigned bits, unsigned dlo = 0, unsigned slo = 0) { RowsWant w; w.bits = bits; w.dense_lo4 = dlo; w.sparse_lo4 = slo; return w; }
static HessWant hwant(unsigned bits, int vdiv = 1) { HessWant w; w.bits = bits; w.vdiv = vdiv; return w; }

static void check_rows_plan(const MfmaShape& s, const RowsWant& w, const MfmaRowsPlan& p) {
    const int MT = s.wp / 16;
    CHECK(p.kernel >= ROW_COOP && p.kernel <= ROW_COOP_SPARSE, "kernel %d", p.kernel);
    CHECK(p.g.grid >= 1 && p.g.wg % 64 == 0 && p.g.wg >= 64 && p.g.wg <= 512, "grid %d wg %d", p.g.grid, p.g.wg);
    unsigned asked = (w.bits & WANT_DENSE ? COVERS_DENSE : 0u) | (w.bits & WANT_SPARSE ? COVERS_SPARSE : 0u) |
                     (w.bits & (WANT_F | WANT_GRAD) ? COVERS_OBJ : 0u) | (w.bits & WANT_GN ? COVERS_GN : 0u);
    CHECK((p.covers & ~asked) == 0, "covers %u of %u", p.covers, asked);
    if (p.family == FAM_FX) {
        CHECK(p.compiled >= 0 && p.compiled < kNumCompiledShapes && kCompiledShapes[p.compiled].kind == CK_FX &&
              compiled_has(kCompiledShapes[p.compiled], s.esz, s.act) && kCompiledShapes[p.compiled].wp == s.wp &&
              kCompiledShapes[p.compiled].nh == s.nh && kCompiledShapes[p.compiled].nx == s.nx, "fx entry %d", p.compiled);
        CHECK(p.tpw == 2 || p.tpw == 3, "tpw %d", p.tpw);
        CHECK(!p.gn || (s.esz == 8 && s.nx == 2), "gn");
        CHECK(p.g.lds_bytes <= (size_t)kLdsBudgetCoop && p.g.wg == MT * 64, "lds %zu", p.g.lds_bytes);
        CHECK(p.g.tiles_per_wg <= 0xff && p.g.tiles_rem <= 0x3ff && p.g.grid <= 0xffff, "packing");
    } else if (p.family == FAM_COOP) {
        CHECK(coop_fits_registers(s.esz, s.wp, s.nh) && s.mb() == 1 && s.ks() <= 4 && s.variant != NEMPC_KERNEL_MFMA_TILE, "coop shape");
        CHECK(p.tpw >= 1 && p.tpw <= (s.wp <= 64 && !p.stage_records ? 3 : 1), "tpw %d", p.tpw);
        CHECK(p.compiled < 0 || (kCompiledShapes[p.compiled].kind == CK_COOP_DIMS && compiled_has(kCompiledShapes[p.compiled], s.esz, s.act) &&
                                 p.tpw == 1), "coop dims entry %d", p.compiled);
        CHECK(p.g.lds_bytes == (size_t)p.lay.total * s.esz && p.g.lds_bytes * p.g.per_cu <= (size_t)kLdsBudgetCoop && p.g.wg == MT * 64,
              "lds %zu x %d", p.g.lds_bytes, p.g.per_cu);
        CHECK(p.stage_records == ((w.bits & WANT_STAGES) != 0), "stage records");
    } else {
        CHECK(p.family == FAM_TILE && p.kernel == ROW_TILE && p.covers == 0, "family %d", p.family);
        CHECK(!p.resident || tile_weights_resident(s.esz, s.wp, s.nh), "resident");
        CHECK(p.waves >= 1 && p.waves <= (p.resident ? kMaxWaves : 4) && p.g.wg == p.waves * 64, "waves %d", p.waves);
        CHECK(p.g.lds_bytes <= (size_t)(p.resident || p.waves > 1 ? kLdsBudget : 160 * 1024), "lds %zu", p.g.lds_bytes);
    }
    CHECK(p.wp == s.wp && p.nh == s.nh, "instantiation");
}

static void check_hess_plan(const MfmaShape& s, const HessWant& w, const MfmaHessPlan& p) {
    const int MT = s.wp / 16;
    if (p.kernel == HESS_NONE) { CHECK(w.bits & HWANT_EVAL, "only an evaluation request may be refused"); return; }
    CHECK(p.g.grid >= 1 && p.g.wg % 64 == 0 && p.g.wg >= 64 && p.g.wg <= 512, "grid %d wg %d", p.g.grid, p.g.wg);
    CHECK(!(p.covers & COVERS_HVALS) || ((w.bits & HWANT_HVALS) && p.family != FAM_TILE), "hvals cover");
    CHECK(((p.covers & COVERS_EVAL) != 0) == ((w.bits & HWANT_EVAL) != 0), "eval cover");
    if (p.family == FAM_FX) {
        const CompiledShape& c = kCompiledShapes[p.compiled < 0 ? 0 : p.compiled];
        CHECK(p.compiled >= 0 && p.compiled < kNumCompiledShapes && (c.kind == CK_FX || c.kind == CK_HESS_DIMS) &&
              compiled_has(c, s.esz, s.act) && c.wp == s.wp && c.nh == s.nh && c.nx == s.nx && c.nu == s.nu, "hessfx entry %d", p.compiled);
        CHECK(!p.ev || c.kind == CK_FX, "ev");
        CHECK(p.g.lds_bytes <= (size_t)kLdsBudgetCoop && p.g.wg == MT * 64, "lds %zu", p.g.lds_bytes);
    } else if (p.family == FAM_COOP) {
        CHECK(coop_fits_registers(s.esz, s.wp, s.nh) && s.mb() == 1 && s.ks() <= 4 && s.variant != NEMPC_KERNEL_MFMA_TILE, "coop shape");
        CHECK(p.g.lds_bytes == (size_t)p.lay.total * s.esz && p.g.lds_bytes * p.g.per_cu <= (size_t)kLdsBudgetCoop && p.g.wg == MT * 64, "lds");
    } else {
        CHECK(p.family == FAM_TILE && p.kernel == HESS_TILE, "family %d", p.family);
        CHECK(!p.resident || tile_weights_resident(s.esz, s.wp, s.nh), "resident");
        CHECK(p.waves >= 1 && p.waves <= 4 && p.g.wg == p.waves * 64, "waves %d", p.waves);
        CHECK(p.g.lds_bytes <= (size_t)(p.resident || p.waves > 1 ? kLdsBudget : 160 * 1024), "lds %zu", p.g.lds_bytes);
    }
}

static void sweep() {
    const MfmaKnobs kn;
    const int acts[] = {NEMPC_ACT_TANH, NEMPC_ACT_RELU, kActRuntime};      // the three classes the table distinguishes
    const unsigned wants[] = {0, WANT_TILES, WANT_TILES | WANT_DENSE, WANT_TILES | WANT_DENSE | WANT_F | WANT_GRAD, WANT_F,
                              WANT_TILES | WANT_F | WANT_GRAD, WANT_SPARSE | WANT_GRAD, WANT_SPARSE, WANT_DENSE | WANT_SPARSE | WANT_F,
                              WANT_TILES | WANT_STAGES, WANT_TILES | WANT_GN};
    const unsigned hwants[] = {HWANT_BLOCKS, HWANT_HVALS, HWANT_BLOCKS | HWANT_EVAL, HWANT_BLOCKS | HWANT_DIRECT};
    const int BH[][2] = {{1, 1}, {1, 16}, {3, 7}, {9, 20}, {64, 20}, {200, 20}, {2000, 20}, {20000, 20}, {70000, 20}};   // one tile .. past every threshold
    long plans = 0;
    for (int esz : {8, 4}) for (int act : acts) for (int wp : {32, 64, 128}) for (int nh = 1; nh <= 4; ++nh) {
        if (nh == 4 && wp > 64) continue;       // (mfma_supported)
        for (int nx = 1; nx <= 16; ++nx) for (int nin = nx + 1; nin <= 32; nin += (nin < 10 ? 1 : 5)) for (int ne : {0, 3}) {
            if (nin + ne > 32) continue;
            for (int integ : {NEMPC_DISCRET, NEMPC_RK4}) for (int variant : {NEMPC_KERNEL_MFMA, NEMPC_KERNEL_MFMA_TILE})
            for (int cus : {1, 4, 256}) for (const auto& bh : BH) {
                const MfmaShape s = shape(esz, wp, nh, nx, nin - nx, ne, integ, variant, act, bh[0], bh[1], cus, nx % 2 == 0);
                if ((size_t)s.rows_scratch() * esz > (size_t)160 * 1024) continue;      // (mfma_supported)
                for (unsigned wb : wants) {
                    if ((wb & WANT_STAGES) && integ != NEMPC_RK4) continue;
                    const RowsWant w = want(wb, (nin & 1) * 8, 0);
                    check_rows_plan(s, w, plan_rows(s, w, kn));
                    ++plans;
                }
                for (unsigned hb : hwants) {
                    if ((hb & HWANT_DIRECT) && integ != NEMPC_RK4) continue;
                    const HessWant w = hwant(hb, 4);
                    check_hess_plan(s, w, plan_hess(s, w, kn));
                    ++plans;
                }
            }
        }
    }
    std::printf("sweep: %ld plans\n", plans);
}

// each refusal that used to happen inside a launcher, on each side of it
static void refusals() {
    const MfmaKnobs kn;
    const int M = NEMPC_KERNEL_MFMA, T = NEMPC_ACT_TANH, D = NEMPC_DISCRET;
    const unsigned ALL = WANT_TILES | WANT_DENSE | WANT_F | WANT_GRAD;
    const MfmaShape c2 = shape(8, 64, 2, 2, 1, 0, D, M, T, 9, 20, 256), s64 = shape(8, 64, 2, 3, 2, 0, D, M, T, 8, 4, 256);
    // 16-byte alignment of the dense / sparse output (compiled shape; cooperative kernel)
    CHECK(plan_rows(c2, want(ALL, 0), kn).covers == (COVERS_DENSE | COVERS_OBJ) && plan_rows(c2, want(ALL, 0), kn).fuse, "aligned dense");
    CHECK(plan_rows(c2, want(ALL, 8), kn).covers == 0 && plan_rows(c2, want(ALL, 8), kn).kernel == ROW_FX, "misaligned dense");
    CHECK(plan_rows(c2, want(WANT_SPARSE | WANT_F, 0, 0), kn).kernel == ROW_FX_SPARSE, "aligned sparse");
    CHECK(plan_rows(c2, want(WANT_SPARSE | WANT_F, 0, 8), kn).kernel == ROW_COOP_SPARSE, "misaligned sparse: the cooperative kernel");
    CHECK(plan_rows(s64, want(ALL, 0), kn).kernel == ROW_COOP_DENSE && plan_rows(s64, want(ALL, 8), kn).kernel == ROW_COOP, "coop dense alignment");
    // rows of whole 16-byte vectors: n a multiple of the vector width (compiled shape), nx * n * esz of 16 (cooperative)
    MfmaShape odd = shape(8, 64, 2, 2, 1, 0, D, M, T, 5, 7, 256);      // n = 21
    CHECK(plan_rows(odd, want(ALL), kn).kernel == ROW_COOP_DENSE, "n %% VEC: compiled shape refuses, cooperative takes (2 * 21 * 8)");
    odd.esz = 4;
    CHECK(plan_rows(odd, want(ALL), kn).kernel == ROW_FX && plan_rows(odd, want(ALL), kn).covers == 0, "fp32: both refuse, tiles from the compiled shape");
    // Gauss-Newton callback: fp64 with two states only (the table has no compiled shape with another nx: the esz side)
    CHECK(plan_rows(c2, want(WANT_TILES | WANT_GN), kn).covers == COVERS_GN && plan_rows(c2, want(WANT_TILES | WANT_GN), kn).gn, "gn fp64");
    MfmaShape c2f = c2; c2f.esz = 4;
    CHECK(plan_rows(c2f, want(WANT_TILES | WANT_GN), kn).covers == 0 && !plan_rows(c2f, want(WANT_TILES | WANT_GN), kn).gn, "gn fp32");
    MfmaShape nos = c2; nos.hess_scatter = false;
    CHECK(plan_rows(nos, want(WANT_TILES | WANT_GN), kn).covers == 0, "gn without the scatter map");
    // the packed per-workgroup tile count: one compute unit, an objective table that leaves room for one workgroup
    MfmaShape big = shape(8, 64, 2, 2, 1, 0, D, M, T, 2, 1500, 1);
    { const MfmaRowsPlan p = plan_rows(big, want(WANT_TILES | WANT_F | WANT_GRAD), kn); CHECK(p.fuse && p.g.per_cu == 1 && p.g.tiles_per_wg == 188, "188 tiles in one workgroup: %d %d", p.g.per_cu, p.g.tiles_per_wg); }
    big.B = 3;
    { const MfmaRowsPlan p = plan_rows(big, want(WANT_TILES | WANT_F | WANT_GRAD), kn); CHECK(!p.fuse && p.kernel == ROW_FX && p.g.tiles_per_wg == 141, "282 tiles: not fused (two workgroups without the table): %d", p.g.tiles_per_wg); }
    big.B = 6;      // 563 tiles > 254 * 2: no compiled shape at all
    CHECK(plan_rows(big, want(WANT_TILES), kn).family != FAM_FX, "past the packed count");
    // (H > 0xffff, a grid > 0xffff and dense rows past 2^31 bytes per pass lie behind B * H * H < 2^32: lines of the plan all the same)
    // rolling windows, stage records: the cooperative kernel writes neither dense rows nor band values
    MfmaShape roll = s64; roll.window = 2; roll.nin = 10;
    CHECK(plan_rows(roll, want(ALL), kn).kernel == ROW_COOP && plan_rows(roll, want(WANT_SPARSE), kn).kernel == ROW_TILE, "rolling");
    CHECK(plan_rows(s64, want(WANT_SPARSE), kn).kernel == ROW_COOP_SPARSE, "plain sparse");
    MfmaShape rk = s64; rk.integrator = NEMPC_RK4;
    CHECK(plan_rows(rk, want(WANT_TILES | WANT_STAGES), kn).stage_records && plan_rows(rk, want(WANT_TILES | WANT_STAGES), kn).tpw == 1, "stage records");
    // the objective without a table
    MfmaShape noobj = s64; noobj.obj_elems = 0;
    CHECK(plan_rows(noobj, want(ALL), kn).kernel == ROW_COOP && plan_rows(noobj, want(WANT_TILES | WANT_DENSE), kn).kernel == ROW_COOP_DENSE, "no table");
    // B * H * H < 2^32 (row / H by multiply-high)
    MfmaShape wide = shape(8, 64, 2, 3, 2, 0, D, M, T, 43, 10000, 1024);
    CHECK(plan_rows(wide, want(WANT_TILES), kn).family == FAM_TILE, "B H H = 4.3e9");
    wide.B = 42;
    CHECK(plan_rows(wide, want(WANT_TILES), kn).family == FAM_COOP, "B H H = 4.2e9");
    // tile-count rule: 32 tiles per compute unit
    MfmaShape one = shape(8, 64, 2, 3, 2, 0, D, M, T, 16, 20, 1);
    CHECK(plan_rows(one, want(WANT_TILES), kn).kernel == ROW_COOP, "20 tiles");
    one.B = 32;
    CHECK(plan_rows(one, want(WANT_TILES), kn).kernel == ROW_TILE && plan_rows(one, want(ALL), kn).kernel == ROW_TILE, "40 tiles");
    // Hessian: blocks + evaluation on a compiled shape only; tril values not from the wave-per-tile kernel
    CHECK(plan_hess(c2, hwant(HWANT_BLOCKS | HWANT_EVAL), kn).covers == COVERS_EVAL && plan_hess(s64, hwant(HWANT_BLOCKS | HWANT_EVAL), kn).kernel == HESS_NONE, "eval");
    CHECK(plan_hess(s64, hwant(HWANT_HVALS), kn).covers == COVERS_HVALS && plan_hess(s64, hwant(HWANT_HVALS), kn).kernel == HESS_COOP, "hvals coop");
    MfmaShape st = s64; st.variant = NEMPC_KERNEL_MFMA_TILE;
    CHECK(plan_hess(st, hwant(HWANT_HVALS), kn).covers == 0 && plan_hess(st, hwant(HWANT_HVALS), kn).kernel == HESS_TILE, "hvals tile");
    MfmaShape lh = s64; lh.layered_hess = true;
    CHECK(plan_hess(lh, hwant(HWANT_HVALS), kn).covers == 0, "hvals on a handle whose blocks are layered");
    const MfmaShape c3 = shape(4, 128, 3, 6, 3, 0, NEMPC_RK4, M, T, 3, 5, 256);
    CHECK(plan_hess(c3, hwant(HWANT_BLOCKS | HWANT_DIRECT, 4), kn).kernel == HESS_FX && plan_hess(c3, hwant(HWANT_BLOCKS), kn).kernel != HESS_FX, "direct mode");
}

// each knob flips the choice its README line names, and nothing else about the plan's kernel
static void knobs() {
    const int M = NEMPC_KERNEL_MFMA, T = NEMPC_ACT_TANH, D = NEMPC_DISCRET;
    const unsigned ALL = WANT_TILES | WANT_DENSE | WANT_F | WANT_GRAD;
    const MfmaShape c2 = shape(8, 64, 2, 2, 1, 0, D, M, T, 9, 20, 256), s64 = shape(8, 64, 2, 3, 2, 0, D, M, T, 8, 4, 256);
    const MfmaShape c3 = shape(4, 128, 3, 6, 3, 0, D, M, T, 5, 6, 256), c3d = shape(8, 128, 3, 6, 3, 0, D, M, T, 5, 6, 256);
    const MfmaKnobs def;
    { MfmaKnobs k; k.fx = false; CHECK(plan_rows(c2, want(ALL), def).kernel == ROW_FX && plan_rows(c2, want(ALL), k).kernel == ROW_COOP_DENSE, "NEMPC_FX");
      CHECK(plan_hess(c2, hwant(HWANT_BLOCKS), k).kernel == HESS_FX, "NEMPC_FX leaves the Hessian"); }
    { MfmaKnobs k; k.hfx = false; CHECK(plan_hess(c2, hwant(HWANT_BLOCKS), def).kernel == HESS_FX && plan_hess(c2, hwant(HWANT_BLOCKS), k).kernel == HESS_COOP, "NEMPC_HFX");
      CHECK(plan_rows(c2, want(ALL), k).kernel == ROW_FX, "NEMPC_HFX leaves the rows"); }
    { MfmaKnobs k; k.hfx_eval = false; CHECK(plan_hess(c2, hwant(HWANT_BLOCKS | HWANT_EVAL), k).kernel == HESS_NONE && plan_hess(c2, hwant(HWANT_BLOCKS), k).kernel == HESS_FX, "NEMPC_HFX_EVAL"); }
    { MfmaKnobs k; k.gn_fused = false; const MfmaRowsPlan p = plan_rows(c2, want(WANT_TILES | WANT_GN), k); CHECK(p.kernel == ROW_FX && !p.gn && p.covers == 0, "NEMPC_GN_FUSED"); }
    { MfmaKnobs k; k.coop_dense = false; CHECK(plan_rows(s64, want(ALL), k).kernel == ROW_COOP && plan_rows(s64, want(WANT_SPARSE), k).kernel == ROW_COOP_SPARSE, "NEMPC_COOP_DENSE"); }
    { MfmaKnobs k; k.coop_sparse = false; CHECK(plan_rows(s64, want(WANT_SPARSE), k).kernel == ROW_TILE && plan_rows(s64, want(ALL), k).kernel == ROW_COOP_DENSE, "NEMPC_COOP_SPARSE"); }
    { MfmaKnobs k; k.coop_dims = false; CHECK(plan_rows(c3, want(WANT_TILES), def).compiled >= 0 && plan_rows(c3, want(WANT_TILES), k).compiled < 0 &&
                                              plan_rows(c3, want(WANT_TILES), k).kernel == ROW_COOP, "NEMPC_COOP_DIMS"); }
    { MfmaKnobs k; k.coop_tpw = 1; MfmaShape f = s64; f.esz = 4; CHECK(plan_rows(f, want(WANT_TILES), def).tpw == 2 && plan_rows(f, want(WANT_TILES), k).tpw == 1, "NEMPC_COOP_TPW"); }
    { MfmaKnobs k; k.fx_tpw = 2; CHECK(plan_rows(c2, want(ALL), def).tpw == 3 && plan_rows(c2, want(ALL), k).tpw == 2, "NEMPC_FX_TPW"); }
    { MfmaKnobs k; k.tile_waves = 2; const MfmaRowsPlan a = plan_rows(c3d, want(WANT_TILES), def), b = plan_rows(c3d, want(WANT_TILES), k);
      CHECK(!a.resident && a.waves == 4 && b.waves == 2 && b.kernel == a.kernel, "NEMPC_TILE_WAVES %d %d", a.waves, b.waves); }
}

static int recorded(const char* path) {
    std::FILE* fh = std::fopen(path, "r");
    if (!fh) { std::printf("cannot open %s\n", path); return 1; }
    char kind[8], id[128];
    int n = 0;
    const MfmaKnobs kn;
    while (std::fscanf(fh, "%7s %127s", kind, id) == 2) {
        MfmaShape s{};
        int hs = 0, lh = 0, code = 0, grid = 0, wg = 0;
        unsigned bits = 0, a = 0, b = 0;
        if (std::fscanf(fh, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %u %u %u %d %d %d", &s.esz, &s.wp, &s.nh, &s.nx, &s.nu,
                        &s.nin, &s.ne, &s.window, &s.integrator, &s.variant, &s.act, &s.n, &s.m, &s.B, &s.H, &s.num_cus, &s.obj_elems,
                        &hs, &lh, &bits, &a, &b, &code, &grid, &wg) != 25) { std::printf("bad line for %s\n", id); std::fclose(fh); return 1; }
        s.hess_scatter = hs; s.layered_hess = lh;
        if (kind[0] == 'R') {
            const RowsWant w = want(bits, a, b);
            const MfmaRowsPlan p = plan_rows(s, w, kn);
            check_rows_plan(s, w, p);
            CHECK(p.kernel == code && p.g.grid == grid && p.g.wg == wg, "%s rows: plan %d grid %d wg %d, recorded %d %d %d", id, p.kernel, p.g.grid, p.g.wg, code, grid, wg);
        } else {
            const HessWant w = hwant(bits, (int)a);
            const MfmaHessPlan p = plan_hess(s, w, kn);
            check_hess_plan(s, w, p);
            CHECK(p.kernel == code && p.g.grid == grid && p.g.wg == wg, "%s hess: plan %d grid %d wg %d, recorded %d %d %d", id, p.kernel, p.g.grid, p.g.wg, code, grid, wg);
        }
        ++n;
    }
    std::fclose(fh);
    std::printf("recorded: %d queries\n", n);
    return 0;
}

template <size_t N>
static void print_names(const char* what, const KernelName (&t)[N]) {
    for (const KernelName& k : t) std::printf("enum %s %d %s\n", what, k.code, k.name[0] ? k.name : "-");
}

int main(int argc, char** argv) {
    print_names("RowKernel", kRowKernelNames);
    print_names("HessKernel", kHessKernelNames);
    std::printf("enum HessKernel+ %d rk4:\n", (int)HESS_IN_RK4);
    print_names("LqKernel", kLqKernelNames);
    print_names("RolloutKernel", kRolloutKernelNames);
    if (argc > 1 && recorded(argv[1])) return 2;
    refusals();
    knobs();
    sweep();
    std::printf("%ld checks, %ld failures\n", checks, failures);
    return failures ? 1 : 0;
}
