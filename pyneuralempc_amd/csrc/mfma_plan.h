// Which register-resident matrix-core kernel serves a request, decided before anything is launched.  Plain C++17, no HIP
// types: tests/plan_check.cpp sweeps it on the CPU.  plan_rows / plan_hess take what of the handle and the call the choice
// depends on (MfmaShape), what the caller asks for (RowsWant / HessWant) and the environment switches (MfmaKnobs); the
// result names the kernel, the instantiation, the launch geometry and what the launch itself writes (`covers`).  The
// typed units (kernels_mfma_typed.inc) only switch from a plan to an instantiation; nobody learns a choice from a
// launcher's return code.
#pragma once

#include <cstddef>
#include <cstdint>

#include "nempc.h"

namespace nempc {

// ---- what ran: the codes nempc_last_*_kernel return (include/nempc.h), with the names engine.py shows
enum RowKernel : int { ROW_NONE, ROW_VALU, ROW_COOP, ROW_TILE, ROW_FX, ROW_COOP_DENSE, ROW_FX_SPARSE, ROW_COOP_SPARSE, ROW_LAYERED };
// HESS_IN_RK4: added to the network kernel's code when it ran inside the RK4 pipeline
enum HessKernel : int { HESS_NONE, HESS_VALU, HESS_COOP, HESS_TILE, HESS_FX, HESS_LAYERED, HESS_IN_RK4 = 10 };
enum LqKernel : int { LQ_NONE, LQ_THREAD_GLOBAL, LQ_THREAD_LDS, LQ_WAVE_LDS, LQ_SCAN };
enum RolloutKernel : int { ROLLOUT_NONE, ROLLOUT_WAVE, ROLLOUT_MFMA };
struct KernelName { int code; const char* name; };       // name "" = none yet
constexpr KernelName kRowKernelNames[] = {
    {ROW_NONE, ""}, {ROW_VALU, "rows_valu_kernel"}, {ROW_COOP, "rows_coop_kernel"}, {ROW_TILE, "rows_mfma_kernel"},
    {ROW_FX, "rows_coopfx_kernel"}, {ROW_COOP_DENSE, "rows_coop_kernel+dense"}, {ROW_FX_SPARSE, "rows_coopfx_kernel+sparse"},
    {ROW_COOP_SPARSE, "rows_coop_kernel+sparse"}, {ROW_LAYERED, "layered_gemm_kernel"}};
constexpr KernelName kHessKernelNames[] = {
    {HESS_NONE, ""}, {HESS_VALU, "rowhess_valu_kernel"}, {HESS_COOP, "rowhess_coop_kernel"}, {HESS_TILE, "rowhess_mfma_kernel"},
    {HESS_FX, "rowhess_coopfx_kernel"}, {HESS_LAYERED, "layered_gemm_kernel"}};
constexpr KernelName kLqKernelNames[] = {
    {LQ_NONE, ""}, {LQ_THREAD_GLOBAL, "thread_global"}, {LQ_THREAD_LDS, "thread_lds"}, {LQ_WAVE_LDS, "wave_lds"}, {LQ_SCAN, "scan"}};
constexpr KernelName kRolloutKernelNames[] = {
    {ROLLOUT_NONE, ""}, {ROLLOUT_WAVE, "rollout_wave_kernel"}, {ROLLOUT_MFMA, "rollout_mfma_kernel"}};

// ---- every environment switch of these launchers (README "Environment switches"), read once per process (mfma_knobs(),
//      kernels_mfma.hip).  All are A/B knobs; the defaults are what ships.
struct MfmaKnobs {
    bool fx = true;           // NEMPC_FX=0: no compiled-shape row kernel
    bool hfx = true;          // NEMPC_HFX=0: no compiled-shape Hessian kernel
    bool hfx_eval = true;     // NEMPC_HFX_EVAL=0: no blocks + first-order evaluation in one launch (batched solver)
    bool gn_fused = true;     // NEMPC_GN_FUSED=0: the Gauss-Newton callback takes the row launch + assembly
    bool coop_dense = true;   // NEMPC_COOP_DENSE=0: the cooperative kernel does not write the dense rows itself
    bool coop_sparse = true;  // NEMPC_COOP_SPARSE=0: ... nor the band values
    bool coop_dims = true;    // NEMPC_COOP_DIMS=0: 6/3 3 x 128 fp32 rows stay off their compiled-dimension cooperative kernel
    static constexpr int kUnset = -1000000;
    int coop_tpw = kUnset;    // NEMPC_COOP_TPW: most tiles per pass of the cooperative kernel (default by shape, coop_tpw_default)
    int fx_tpw = 3;           // NEMPC_FX_TPW: 3 | 2 tiles per pass of the compiled-shape row kernel
    int tile_waves = 4;       // NEMPC_TILE_WAVES: waves per workgroup of the streamed wave-per-tile kernel (1 .. 4)
};

// ---- launch geometry of the cooperative kernels: `per_cu` co-resident workgroups on each of the device's `num_cus`
// compute units (fewer when there are fewer tiles), each owning a contiguous run of tiles_per_wg (+1 for the first
// tiles_rem workgroups) 16-row tiles.  num_cus comes from hipDeviceProp_t::multiProcessorCount of the handle's device
// (256 on an MI355X in SPX mode; a partitioned mode or another gfx950 part reports its own count).
struct GridPlan {
    int grid, tiles_per_wg, tiles_rem;
};
inline GridPlan plan_grid(int ntiles, int num_cus, int per_cu) {
    long long g = (long long)(num_cus < 1 ? 1 : num_cus) * (per_cu < 1 ? 1 : per_cu);
    if (g > ntiles) g = ntiles;
    if (g < 1) g = 1;
    return GridPlan{(int)g, ntiles / (int)g, ntiles % (int)g};
}

constexpr int kActRuntime = 100;     // NEMPC_ACT_RUNTIME (activations.h): per-layer codes at run time
constexpr int kMfmaMaxHidden = 4;    // NEMPC_MFMA_MAX_HIDDEN
constexpr int kMaxKs = 8;            // first-layer k-steps: network inputs (window + extras) up to 32
constexpr int kLdsBudget = 150 * 1024;       // wave-per-tile kernels, of the CU's 160 KiB
constexpr int kLdsBudgetCoop = 160 * 1024;   // cooperative kernels
constexpr int kMaxWaves = 8;                 // 512 threads: keeps 256 VGPRs per lane available
constexpr int kHessTG = 3;                   // tangent directions swept together by the cooperative Hessian kernel
constexpr int kFxZcopy = 512;                // FX_ZCOPY (kernels_coopfx_impl.h)
constexpr int up16(int v) { return (v + 15) & ~15; }

struct MfmaOffsets {  // element offsets into the packed blob
    int w0f, wLf, w0b, seed, biasL;
    int p0tab, wLb;  // Hessian kernel tables: first-layer rows W_0[p,:], output-layer fragments for W_L lambda
    int wf[kMfmaMaxHidden], wb[kMfmaMaxHidden], bias[kMfmaMaxHidden];
    int total;
    // cooperative row kernel: the same numbers once more, laid out for its prologue (kernels_coop_impl.h) --
    //   coop_small   [w0f | seed | bias_l | biasL] contiguous (one flat copy to LDS),
    //   coop_slices  per wave: its register-resident fragments (wf, wb per hidden layer, wL, w0b) as 16-byte
    //                lane vectors, load k of lane = element ((wave * coop_nload + k) * 64 + lane) * VEC
    int coop_small, coop_small_elems, coop_slices, coop_nload;
    //   fx_small     [w0f | seed | bias_l | biasL | p0tab]: the fixed-shape kernel's tables (p0tab = first-layer rows per
    //                lane, for its vector-unit skinny layers)
    int fx_small, fx_small_elems;
    int grand_total;
};

inline MfmaOffsets make_offsets(int wp, int nh, int ks, int nx, int nin, int esz) {
    const int MT = wp / 16;
    MfmaOffsets o{};
    int p = 0;
    o.w0f = p; p += ks * MT * 64;
    for (int l = 1; l < nh; ++l) { o.wf[l] = p; p += MT * MT * 4 * 64; }
    o.wLf = p; p += MT * 4 * 64;
    for (int l = 1; l < nh; ++l) { o.wb[l] = p; p += MT * MT * 4 * 64; }
    o.w0b = p; p += MT * 4 * 64 * ((nin + 15) / 16);   // one fragment set per 16-row block of the input dimension
    o.p0tab = p; p += nin * MT * 16;
    o.wLb = p; p += ((nx + 3) / 4) * MT * 64;
    o.seed = p; p += nx * MT * 16;
    for (int l = 0; l < nh; ++l) { o.bias[l] = p; p += MT * 16; }
    o.biasL = p; p += 16;
    o.total = p;
    // cooperative-kernel copies (16-byte aligned: every size above is a multiple of 16 elements)
    const int vec = 16 / esz;
    const int nfrag = (nh - 1) * 2 * MT * 4 + 8;
    o.coop_small = p;
    o.coop_small_elems = ks * MT * 64 + (o.total - o.seed);
    p += (o.coop_small_elems + 15) & ~15;
    o.coop_nload = (nfrag + vec - 1) / vec;
    o.coop_slices = p;
    p += MT * o.coop_nload * 64 * vec;
    o.fx_small = p;
    o.fx_small_elems = o.coop_small_elems + nin * MT * 16;
    p += (o.fx_small_elems + 15) & ~15;
    o.grand_total = p;
    return o;
}

// ---- the cooperative kernels' LDS (element offsets inside dynamic LDS) and the three small functions it is sized by
// (constexpr: the device code calls them too).
// Cotangents swept together in the reverse pass: two when their accumulators are no bigger than those of a 2-tile
// fp64 pass (fp64: single-tile passes; fp32: passes of <= 2 tiles).  Two independent MFMA chains per wave and half the
// exchange barriers -- what the latency-bound cases (single-tile passes, 8-wave workgroups) lack.
template <typename T>
constexpr int coop_kg(int NT) {
#ifdef NEMPC_EXP_KG1
    return 1;
#endif
    return NT * (int)sizeof(T) <= 8 ? 2 : 1;   // three at a time for fp32 single-tile passes measured no better (576 vs 568 us at C3)
}
// exchange-buffer slots (16-row activation sets) a pass may publish at once
template <typename T>
constexpr int coop_slots(int TPW) {
    int m = 0;
    for (int nt = 1; nt <= TPW; ++nt) m = nt * coop_kg<T>(nt) > m ? nt * coop_kg<T>(nt) : m;
    return m;
}
template <typename T>
constexpr int coop_nr(int nin) { return sizeof(T) == 8 ? (nin + 3) / 4 : 4; }      // accumulator registers holding the nin input rows

struct CoopLayout {  // rows_coop_kernel
    int w0f;         // layer-0 fragments          ks * MT * 64          [w0f | tail] contiguous: one flat copy of off.coop_small
    int tail;        // seed | bias_l | biasL      (off.total - off.seed)
    int x;           // exchange buffer            2 halves of slots * MT * 256
    int xhalf;
    int part;        // partials                   (1+nx) * TPW * MT * NR * 64
    int scratch, scratch2;   // per-tile scratch   TPW * scratch_per_wave, twice (the second: next pass's inputs)
    int rowinfo, rowinfo2;   // (b, t) per tile row as int2  TPW * 16 * 2 ints (stored in T-sized slots), twice
    int total;
};
struct HessCoopLayout {  // rowhess_coop_kernel
    int w0f;             // layer-0 fragments                               ks * MT * 64
    int tail;            // p0tab | wLb | seed | bias_l | biasL             off.total - off.p0tab
    int x, xhalf;        // exchange buffer: 2 halves of TG * MT * 256
    int part;            // K-split partials of the Hessian columns         TG * MT * NR * 64
    int scratch;         // xi0[16][nin] | lam[16][nx] | ex[16][ne] | H[16][nin][nin]
    int total;
};

// ---- the compiled shapes: ONE table.  The typed units instantiate from it (an index sequence with `if constexpr` on the
// unit's dtype and activation); the plans match against it.
//   CK_FX         rows_coopfx_kernel (plain, fused evaluation, Gauss-Newton callback in fp64 with two states) and
//                 rowhess_coopfx_kernel: plain Discret / Unity models.  Every compiled activation in fp64 for BASELINE
//                 configs[1] / configs[4] (2/1, 2 x 64); tanh only for the reference's own example network 3 -> 30 -> 30 -> 2
//                 (examples/lotka_volterra/run.py:64-98: padded width 32) in both precisions, and 2/1 2 x 64 in fp32
//   CK_COOP_DIMS  rows_coop_kernel with nx / nu as compile-time constants (BASELINE configs[2]: 6/3, 3 x 128, fp32)
//   CK_HESS_DIMS  rowhess_coopfx_kernel of the same dims, three tangent directions per exchange: the Discret / Unity blocks
//                 and the (row, stage) pairs of the RK4 pipeline (direct mode)
enum CompiledKind : int { CK_FX, CK_COOP_DIMS, CK_HESS_DIMS };
enum ActSet : int { ACTS_NONE, ACTS_TANH, ACTS_COMPILED /* all but run-time codes */, ACTS_ANY };
struct CompiledShape {
    int kind, wp, nh, nx, nu;
    int acts_f64, acts_f32;
};
constexpr CompiledShape kCompiledShapes[] = {
    {CK_FX, 64, 2, 2, 1, ACTS_COMPILED, ACTS_TANH},
    {CK_FX, 32, 2, 2, 1, ACTS_TANH, ACTS_TANH},
    {CK_COOP_DIMS, 128, 3, 6, 3, ACTS_NONE, ACTS_ANY},
    {CK_HESS_DIMS, 128, 3, 6, 3, ACTS_NONE, ACTS_COMPILED},
};
constexpr int kNumCompiledShapes = (int)(sizeof(kCompiledShapes) / sizeof(kCompiledShapes[0]));
constexpr bool compiled_has(const CompiledShape& c, int esz, int act) {
    const int set = esz == 8 ? c.acts_f64 : c.acts_f32;
    return set == ACTS_ANY || (set == ACTS_COMPILED && act != kActRuntime) || (set == ACTS_TANH && act == NEMPC_ACT_TANH);
}

// LDS elements of the compiled-shape kernels (FxLayout / HfxLayout ::TOTAL; the typed units static_assert the equality)
constexpr int fx_lds_elems(int wp, int nh, int tpw, int nx, int nu) {
    const int MT = wp / 16, nin = nx + nu, ks = (nin + 3) / 4;
    const int small_end = ks * MT * 64 + nx * MT * 16 + nh * MT * 16 + 16 + nin * MT * 16;
    const int part = up16(small_end) + 2 * tpw * MT * 256;
    const int in = part + tpw * MT * nx * 16 + nx * tpw * MT * nin * 16;
    return in + 2 * up16(tpw * 16 * (nin + nx));
}
constexpr int hfx_lds_elems(int wp, int nh, int nt, int nx, int nu, int tg, bool ev) {
    const int MT = wp / 16, nin = nx + nu, ks = (nin + 3) / 4, npair = nin * (nin + 1) / 2;
    const int nvt = npair + (ev ? nx * nin + nx : 0);
    const int small_end = ks * MT * 64 + nx * MT * 16 + nh * MT * 16 + 16 + nin * MT * 16;
    const int x = up16(up16(small_end) + npair * MT * 16);
    const int in = x + 2 * nt * tg * MT * 256 + up16(MT * nt * nvt * 16);
    return in + 2 * up16(nt * 16 * (nin + nx));
}

// register budget of the cooperative kernels' weight slices: (NH-1) * 2 * MT*4 + 8 values per lane
constexpr bool coop_fits_registers(int esz, int wp, int nh) { return ((nh - 1) * 2 * (wp / 16) * 4 + 8) * (esz / 4) <= 144; }
// hidden-to-hidden fragment arrays of the wave-per-tile kernels: resident in LDS up to 96 KiB (they must leave room for the
// rest of the blob and the per-wave scratch), else streamed
constexpr bool tile_weights_resident(int esz, int wp, int nh) {
    return (size_t)(nh - 1) * 2 * (wp / 16) * (wp / 16) * 256 * esz <= 96 * 1024;
}
// passes of <= 3 tiles: the 4-tile instantiation sits at the 256-VGPR cap of two waves per SIMD and spills.  fp64 2 x 64 and
// larger: so does the 3-tile one; measured 21.2 us against 20.4 us for 2-tile passes at C2 dims (B=1024)
constexpr int coop_tpw_default(int esz, int wp, int nh) { return (esz == 8 && wp >= 64 && nh >= 2) ? 2 : 3; }

// ---- what the choice depends on, of the handle and the call
struct MfmaShape {
    int esz, wp, nh;                 // element size, padded width, hidden layers
    int nx, nu, nin, ne, window;     // nin = window * (nx + nu)
    int integrator, variant, act;    // NEMPC_DISCRET .. | NEMPC_KERNEL_MFMA[_TILE] | the hidden activation (kActRuntime: per layer)
    int n, m, B, H, num_cus;
    int obj_elems;                   // elements of the objective table, 0: none set
    bool hess_scatter;               // the Hessian map has its scatter form (plain models)
    bool layered_hess;               // the handle's Lagrangian blocks come from the layered sweeps
    int ks() const { return (nin + ne + 3) / 4; }
    int mb() const { return (nin + 15) / 16; }
    MfmaOffsets offsets() const { return make_offsets(wp, nh, ks(), nx, nin, esz); }
    // one wave's scratch of the row kernels: xi0 | k | acck | J [| dk | accdk | dkn : RK4 chain only] | x_t slot (cooperative
    // kernel) | extra inputs
    int rows_scratch() const {
        const int njs = integrator == NEMPC_RK4 ? 4 : 1;
        return (16 * nin + 2 * 16 * nx + njs * 16 * nx * nin + 16 * nx + 16 * ne + 1) & ~1;
    }
    int hess_scratch() const { return (16 * nin + 16 * nx + 16 * nin * nin + 16 * ne + 1) & ~1; }
};

enum : unsigned {       // RowsWant::bits
    WANT_TILES = 1,     // the compact tiles (the caller's, or for an assembly launch behind this one)
    WANT_DENSE = 2, WANT_SPARSE = 4, WANT_F = 8, WANT_GRAD = 16,
    WANT_STAGES = 32,   // stage records (RK4 Hessian pipeline)
    WANT_GN = 64,       // Gauss-Newton tril values
};
struct RowsWant {
    unsigned bits = 0;
    unsigned dense_lo4 = 0, sparse_lo4 = 0;    // low four address bits of the dense / sparse output
};
enum : unsigned {       // HessWant::bits
    HWANT_BLOCKS = 1, HWANT_HVALS = 2,   // HVALS: tril values and nothing else (the kernel assembles them where it can)
    HWANT_EVAL = 4,                      // blocks plus the first-order evaluation (defects, tiles) of the same rows
    HWANT_DIRECT = 8,                    // direct mode: (row, stage) records instead of Z (RK4 pipeline), vdiv records per row
};
struct HessWant {
    unsigned bits = 0;
    int vdiv = 1;
};
enum : unsigned { COVERS_DENSE = 1, COVERS_SPARSE = 2, COVERS_OBJ = 4, COVERS_GN = 8, COVERS_HVALS = 16, COVERS_EVAL = 32 };
enum MfmaFamily : int { FAM_NONE, FAM_FX, FAM_COOP, FAM_TILE };

struct LaunchGeom {
    int grid = 0, wg = 0, per_cu = 0;   // workgroups, threads per workgroup, workgroups per CU the grid was sized for
    size_t lds_bytes = 0;
    int tiles_per_wg = 0, tiles_rem = 0;
};
struct MfmaRowsPlan {
    int kernel = ROW_NONE;      // ROW_NONE: not ours
    int family = FAM_NONE;
    int wp = 0, nh = 0;         // COOP, TILE: the instantiation's padded width and hidden layers
    int compiled = -1;          // FX, COOP with compiled dims: index into kCompiledShapes
    int tpw = 0;                // FX, COOP: tiles per pass
    bool fuse = false, gn = false;   // FX: the fused-evaluation / Gauss-Newton instantiation
    bool stage_records = false;      // COOP
    bool resident = false;           // TILE: weights in LDS (else streamed)
    int waves = 0;                   // TILE
    int zp_max = 0;                  // FX fused: problems whose variables fit the LDS copy
    unsigned covers = 0;             // COVERS_*: what the launch itself writes
    LaunchGeom g;
    CoopLayout lay{};
};
struct MfmaHessPlan {
    int kernel = HESS_NONE;     // HESS_NONE: not ours
    int family = FAM_NONE;
    int wp = 0, nh = 0;
    int compiled = -1;
    bool ev = false;            // FX: blocks + first-order evaluation
    bool resident = false;
    int waves = 0;
    unsigned covers = 0;        // COVERS_HVALS | COVERS_EVAL
    LaunchGeom g;
    HessCoopLayout lay{};
};

inline int find_compiled(int kind, const MfmaShape& s) {
    for (int i = 0; i < kNumCompiledShapes; ++i) {
        const CompiledShape& c = kCompiledShapes[i];
        if (c.kind == kind && c.wp == s.wp && c.nh == s.nh && c.nx == s.nx && c.nu == s.nu && s.nin == c.nx + c.nu &&
            s.window == 1 && compiled_has(c, s.esz, s.act))
            return i;
    }
    return -1;
}

inline CoopLayout coop_layout(const MfmaShape& s, int tpw) {
    const int MT = s.wp / 16, ks = s.ks(), spw = s.rows_scratch();
    const MfmaOffsets off = s.offsets();
    const int NR = s.esz == 8 ? coop_nr<double>(s.nin) : coop_nr<float>(s.nin);
    const int slots = s.esz == 8 ? coop_slots<double>(tpw) : coop_slots<float>(tpw);
    CoopLayout lay{};
    int q = 0;
    lay.w0f = q; q += ks * MT * 64;
    lay.tail = q; q += up16(off.total - off.seed);
    lay.x = q; lay.xhalf = slots * MT * 256; q += 2 * lay.xhalf;
    lay.part = q; q += up16((1 + s.nx) * tpw * MT * NR * 64);
    lay.scratch = q; q += up16(tpw * spw);
    lay.scratch2 = q; q += up16(tpw * spw);
    lay.rowinfo = q; q += up16(tpw * 16 * 2 * (int)sizeof(int) / s.esz + 1);
    lay.rowinfo2 = q; q += up16(tpw * 16 * 2 * (int)sizeof(int) / s.esz + 1);
    lay.total = q;
    return lay;
}

inline HessCoopLayout hess_coop_layout(const MfmaShape& s) {
    const int MT = s.wp / 16;
    const MfmaOffsets off = s.offsets();
    const int NR = s.esz == 8 ? coop_nr<double>(s.nin) : coop_nr<float>(s.nin);
    HessCoopLayout lay{};
    int q = 0;
    lay.w0f = q; q += up16(s.ks() * MT * 64);
    lay.tail = q; q += up16(off.total - off.p0tab);
    lay.x = q; lay.xhalf = kHessTG * MT * 256; q += 2 * lay.xhalf;
    lay.part = q; q += up16(kHessTG * MT * NR * 64);
    lay.scratch = q; q += up16(16 * (s.nin + s.nx + s.ne + s.nin * s.nin));
    lay.total = q;
    return lay;
}

inline void set_coop_geom(LaunchGeom& g, int ntiles, int num_cus, int per_cu, int MT, size_t bytes) {
    const GridPlan gp = plan_grid(ntiles, num_cus, per_cu);
    g.grid = gp.grid; g.wg = MT * 64; g.per_cu = per_cu; g.lds_bytes = bytes;
    g.tiles_per_wg = gp.tiles_per_wg; g.tiles_rem = gp.tiles_rem;
}

// wave-per-tile geometry, rows and Hessian alike: weights resident in LDS when they fit next to the per-wave scratch (one
// workgroup per CU, as many waves -- up to max_waves -- as it takes to cover the tiles), else streamed with `streamed_waves`
// waves per workgroup, halved while their scratch does not fit
inline void set_tile_geom(const MfmaShape& s, int ntiles, int scratch_elems, int max_waves, int streamed_waves, bool& resident,
                          int& waves, LaunchGeom& g) {
    const size_t blob_bytes = (size_t)((s.offsets().total + 1) & ~1) * s.esz, scratch = (size_t)scratch_elems * s.esz;
    g.per_cu = 1; g.tiles_per_wg = g.tiles_rem = 0;
    if (tile_weights_resident(s.esz, s.wp, s.nh)) {
        waves = (ntiles + s.num_cus - 1) / s.num_cus;
        waves = waves < 1 ? 1 : (waves > max_waves ? max_waves : waves);
        if (blob_bytes + (size_t)waves * scratch <= (size_t)kLdsBudget) {
            resident = true;
            g.grid = (ntiles + waves - 1) / waves;
            if (g.grid > s.num_cus) g.grid = s.num_cus;
            g.wg = waves * 64; g.lds_bytes = blob_bytes + waves * scratch;
            return;
        }
    }
    resident = false;
    waves = streamed_waves < 1 ? 1 : (streamed_waves > 4 ? 4 : streamed_waves);
    while (waves > 1 && (size_t)waves * scratch > (size_t)kLdsBudget) waves >>= 1;
    g.grid = (ntiles + waves - 1) / waves;
    g.wg = waves * 64; g.lds_bytes = (size_t)waves * scratch;
}

// Rows.  Order of preference: compiled shape (whole evaluation / Gauss-Newton callback in one launch), cooperative kernel
// writing the dense rows or the band values itself, compiled shape for the tiles, cooperative kernel, wave-per-tile kernel.
// The wave-per-tile kernel takes every shape the handle was created with, so a row request is always ours.  WANT_GN comes
// with WANT_TILES: without COVERS_GN the caller assembles the values from the tiles.
inline MfmaRowsPlan plan_rows(const MfmaShape& s, const RowsWant& w, const MfmaKnobs& kn) {
    const int MT = s.wp / 16, VEC = 16 / s.esz;
    const int ntiles = (int)(((size_t)s.B * s.H + 15) / 16);
    const bool tiles = w.bits & WANT_TILES, dense = w.bits & WANT_DENSE, sparse = w.bits & WANT_SPARSE;
    const bool obj = w.bits & (WANT_F | WANT_GRAD), stages = w.bits & WANT_STAGES;
    const bool mfma = s.variant == NEMPC_KERNEL_MFMA, plain = s.window == 1;
    // the cooperative kernels: not under NEMPC_KERNEL_MFMA_TILE (A/B), inputs on one 16-row block and four k-steps, and
    // row / H by multiply-high
    const bool coop_shape = s.variant != NEMPC_KERNEL_MFMA_TILE && s.mb() == 1 && s.ks() <= 4 &&
                            (unsigned long long)s.B * s.H * s.H < 0x100000000ull;
    // compiled shape: plain Discret / Unity models without extra inputs; the packed per-workgroup tile count holds 255
    const int fx = kn.fx && coop_shape && !stages && s.ne == 0 && s.integrator != NEMPC_RK4 &&
                           ntiles <= 254 * (8 / MT) * s.num_cus ? find_compiled(CK_FX, s) : -1;

    auto fx_plan = [&](bool fuse, bool gn, unsigned covers, int code) {
        const CompiledShape& c = kCompiledShapes[fx];
        MfmaRowsPlan p;
        p.wp = s.wp; p.nh = s.nh;
        p.tpw = kn.fx_tpw >= 3 ? 3 : 2;
        const int p_elems = fuse ? s.obj_elems : 0;
        const size_t bytes = (size_t)(fx_lds_elems(c.wp, c.nh, p.tpw, c.nx, c.nu) + up16(p_elems) + (fuse ? 2 * kFxZcopy : 0)) * s.esz;
        int per_cu = (int)((size_t)kLdsBudgetCoop / bytes);
        if (per_cu > 8 / MT) per_cu = 8 / MT;
        if (per_cu < 1) per_cu = 1;
        set_coop_geom(p.g, ntiles, s.num_cus, per_cu, MT, bytes);
        // the objective table must be complete in LDS before the first pass for the LDS-resident problems (and a side's copy
        // of Z is fetched as two elements per thread)
        p.zp_max = fuse && p_elems <= 2 * MT * 64 ? (kFxZcopy < 2 * MT * 64 ? kFxZcopy : 2 * MT * 64) / s.n : 0;
        // the background zeros of a pass's dense rows leave as flat runs of 16-byte vectors with 32-bit byte offsets
        if (fuse && dense && (s.n / VEC < 1 || s.n % VEC != 0 || (size_t)(p.tpw * 16 * c.nx) * s.n * s.esz >= 0x7fffffffull)) return MfmaRowsPlan{};
        // what travels packed in the preloaded leading arguments
        if (p.g.tiles_per_wg > 0xff || p.g.tiles_rem > 0x3ff || p.zp_max > 0x3ff || s.n != s.H * (c.nx + c.nu) || s.H > 0xffff ||
            p.g.grid > 0xffff)
            return MfmaRowsPlan{};
        p.kernel = code; p.family = FAM_FX; p.compiled = fx; p.fuse = fuse; p.gn = gn; p.covers = covers;
        return p;
    };
    auto coop_try = [&](MfmaRowsPlan& p, int tpw) {
        const CoopLayout lay = coop_layout(s, tpw);
        const size_t bytes = (size_t)lay.total * s.esz;
        const int wg_by_regs = 8 / MT;      // __launch_bounds__(MT*64, 2): two waves per SIMD
        int per_cu = (int)((size_t)kLdsBudgetCoop / bytes);
        if (per_cu < 1) return false;
        if (per_cu > wg_by_regs) per_cu = wg_by_regs;
        if (per_cu < wg_by_regs && tpw > 1) return false;   // prefer a smaller pass that keeps two waves per SIMD
        p.tpw = tpw; p.lay = lay;
        set_coop_geom(p.g, ntiles, s.num_cus, per_cu, MT, bytes);
        return true;
    };
    auto coop_plan = [&](unsigned covers, int code) {
        MfmaRowsPlan p;
        p.wp = s.wp; p.nh = s.nh;
        if (!coop_shape || !coop_fits_registers(s.esz, s.wp, s.nh)) return p;
        bool ok = false;
        if (stages) {
            ok = coop_try(p, 1);        // the stage-record instantiation, one tile per pass
        } else {
            // Beyond ~8 tiles per SIMD the wave-per-tile kernel with two waves per SIMD is ahead (B=16384, C2 dims:
            // 209 us vs 238 us); below, the cooperative kernel's even split wins (B=256: 12.9 vs 16.5 us).
            if (tile_weights_resident(s.esz, s.wp, s.nh) && ntiles > 32 * s.num_cus) return p;
            if (s.wp <= 64) {
                const int cap = kn.coop_tpw == MfmaKnobs::kUnset ? coop_tpw_default(s.esz, s.wp, s.nh) : kn.coop_tpw;
                ok = (cap >= 3 && coop_try(p, 3)) || (cap >= 2 && coop_try(p, 2));
            }
            // width 128 = 8 waves per workgroup (two per SIMD): one tile per pass is what LDS and registers allow
            if (!ok) ok = coop_try(p, 1);
        }
        if (!ok) return MfmaRowsPlan{};
        if (p.tpw == 1 && kn.coop_dims) p.compiled = find_compiled(CK_COOP_DIMS, s);
        p.kernel = code; p.family = FAM_COOP; p.stage_records = stages; p.covers = covers;
        return p;
    };

    if ((w.bits & WANT_GN) && kn.gn_fused && mfma && plain && s.hess_scatter && s.esz == 8 && fx >= 0 && s.nx == 2) {
        // (the epilogue sums the two states by a quad permute)
        const MfmaRowsPlan p = fx_plan(false, true, COVERS_GN, ROW_FX);
        if (p.kernel) return p;
    }
    if (mfma && fx >= 0 && s.obj_elems > 0) {       // rows, objective and the dense rows / band values in ONE launch
        if (!sparse && (dense || obj) && !(dense && (s.n % VEC != 0 || w.dense_lo4 != 0))) {
            const MfmaRowsPlan p = fx_plan(true, false, (dense ? COVERS_DENSE : 0u) | (obj ? COVERS_OBJ : 0u), ROW_FX);
            if (p.kernel) return p;
        }
        if (sparse && !dense && w.sparse_lo4 == 0) {
            const MfmaRowsPlan p = fx_plan(true, false, COVERS_SPARSE | (obj ? COVERS_OBJ : 0u), ROW_FX_SPARSE);
            if (p.kernel) return p;
        }
    }
    // the cooperative kernel fuses the objective only together with the dense rows or the band values (plain models)
    if (mfma && !stages && plain && (!obj || s.obj_elems > 0)) {
        if (sparse && !dense && kn.coop_sparse) {
            const MfmaRowsPlan p = coop_plan(COVERS_SPARSE | (obj ? COVERS_OBJ : 0u), ROW_COOP_SPARSE);
            if (p.kernel) return p;
        }
        // row blocks of whole 16-byte vectors; flat zero runs with 32-bit byte offsets
        const size_t blk = (size_t)s.nx * s.n * s.esz;
        if (dense && !sparse && kn.coop_dense && blk % 16 == 0 && w.dense_lo4 == 0 && 4 * 16 * blk < 0x7fffffffull) {
            const MfmaRowsPlan p = coop_plan(COVERS_DENSE | (obj ? COVERS_OBJ : 0u), ROW_COOP_DENSE);
            if (p.kernel) return p;
        }
    }
    if (tiles && fx >= 0) {
        const MfmaRowsPlan p = fx_plan(false, false, 0, ROW_FX);
        if (p.kernel) return p;
    }
    if (tiles) {        // (defect-only launches take the wave-per-tile kernel)
        const MfmaRowsPlan p = coop_plan(0, ROW_COOP);
        if (p.kernel) return p;
    }
    MfmaRowsPlan p;
    p.wp = s.wp; p.nh = s.nh;
    p.kernel = ROW_TILE; p.family = FAM_TILE;
    set_tile_geom(s, ntiles, s.rows_scratch(), kMaxWaves, kn.tile_waves, p.resident, p.waves, p.g);
    return p;
}

// Lagrangian blocks.  Order of preference: compiled shape, cooperative kernel, wave-per-tile kernel.  The tril values leave
// from the kernel itself (COVERS_HVALS) on the first two, plain models; blocks + first-order evaluation in one launch
// (HWANT_EVAL) exists for the compiled shapes only -- otherwise not ours.
inline MfmaHessPlan plan_hess(const MfmaShape& s, const HessWant& w, const MfmaKnobs& kn) {
    const int MT = s.wp / 16;
    const bool direct = w.bits & HWANT_DIRECT, ev = w.bits & HWANT_EVAL;
    const int vd = direct ? w.vdiv : 1;
    const int ntiles = (int)(((size_t)s.B * s.H * vd + 15) / 16);
    const bool hvals = (w.bits & HWANT_HVALS) && !direct && s.window == 1 && s.hess_scatter && !s.layered_hess;
    // NEMPC_KERNEL_MFMA_TILE keeps the wave-per-tile Hessian kernel (A/B measurements), like it does for the rows
    const bool allow_coop = s.variant != NEMPC_KERNEL_MFMA_TILE && s.mb() == 1 && s.ks() <= 4;
    MfmaHessPlan p;
    p.wp = s.wp; p.nh = s.nh;
    if (ev && !(kn.hfx_eval && s.window == 1 && s.ne == 0)) return p;
    auto fx_plan = [&](int idx, int tg, bool with_ev) {
        const CompiledShape& c = kCompiledShapes[idx];
        const size_t bytes = (size_t)hfx_lds_elems(c.wp, c.nh, 1, c.nx, c.nu, tg, with_ev) * s.esz;
        int per_cu = (int)((size_t)kLdsBudgetCoop / bytes);
        if (per_cu > 8 / MT) per_cu = 8 / MT;
        if (per_cu < 1) per_cu = 1;
        set_coop_geom(p.g, ntiles, s.num_cus, per_cu, MT, bytes);
        p.kernel = HESS_FX; p.family = FAM_FX; p.compiled = idx; p.ev = with_ev;
        p.covers = (hvals ? COVERS_HVALS : 0u) | (with_ev ? COVERS_EVAL : 0u);
    };
    if (kn.hfx && allow_coop && s.ne == 0) {
        const int fx = s.integrator != NEMPC_RK4 && !direct && (unsigned long long)s.B * s.H * s.H < 0x100000000ull
                           ? find_compiled(CK_FX, s) : -1;
        if (fx >= 0) { fx_plan(fx, s.nx + s.nu, ev); return p; }
        const int c3 = !ev && (direct || s.integrator != NEMPC_RK4) && (unsigned long long)s.B * s.H * s.H * vd < 0x100000000ull
                           ? find_compiled(CK_HESS_DIMS, s) : -1;
        if (c3 >= 0) { fx_plan(c3, 3, false); return p; }
    }
    if (ev) return p;
    if (allow_coop && coop_fits_registers(s.esz, s.wp, s.nh)) {
        const HessCoopLayout lay = hess_coop_layout(s);
        const size_t bytes = (size_t)lay.total * s.esz;
        int per_cu = (int)((size_t)kLdsBudgetCoop / bytes);
        if (per_cu >= 1) {
            if (per_cu > 8 / MT) per_cu = 8 / MT;       // __launch_bounds__(MT*64, 2)
            set_coop_geom(p.g, ntiles, s.num_cus, per_cu, MT, bytes);
            p.kernel = HESS_COOP; p.family = FAM_COOP; p.lay = lay; p.covers = hvals ? COVERS_HVALS : 0u;
            return p;
        }
    }
    // one wave per SIMD: the kernel needs > 256 registers
    p.kernel = HESS_TILE; p.family = FAM_TILE;
    set_tile_geom(s, ntiles, s.hess_scratch(), 4, 4, p.resident, p.waves, p.g);
    return p;
}

}  // namespace nempc
