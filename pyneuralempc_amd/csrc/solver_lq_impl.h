// Batched solver, LQ solve by a Riccati sweep with a thread per problem (LDS or global temporaries), and the staging and
// post-pass that the scan variant shares.  Included by solver.hip only.
#pragma once

namespace nempc {

namespace {

// 1 / sqrt(d) for a pivot d > 1e-12: hardware estimate + two coupled Newton steps (double; ~1 ulp) or one (float).  The
// IEEE sqrt followed by the IEEE division is ~32 instructions of a chain that a lone lane issues one per ~10 cycles.
__device__ __forceinline__ double inv_sqrt_pos(double d) {
    const double y = __builtin_amdgcn_rsq(d);
    double g = d * y, h = 0.5 * y;
    double r = fma(-g, h, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    r = fma(-g, h, 0.5);
    h = fma(h, r, h);
    return h + h;
}
__device__ __forceinline__ float inv_sqrt_pos(float d) {
    const float y = __builtin_amdgcn_rsqf(d);
    const float r = fmaf(-d * y, y, 1.0f);
    return fmaf(0.5f * y, r, y);
}

// Accumulator of the sweeps' sums (products of the value function, the tiles and the steps; shared with solver_lqw_impl.h).
// Stages whose dimensions are compile-time constants sum 2 .. 6 terms per entry and keep T.  The run-time-dimension
// instantiation serves the wide stages, where an entry is a sum over up to nx terms: in fp32 at 64 states that sum alone
// lost more than ten times what a NumPy float32 sweep loses on the same step (the rows 64x8_fp32 of
// tests/solver_step_cases.py missed their tolerances by 1.28 and 1.11; a CPU float32 replay of the kernel's order reproduces
// the device's figures to three digits), so there it runs in double and is rounded to T once per entry.  T = double: no change.
template <typename T, int NX> struct LqAcc { using type = T; };
template <> struct LqAcc<float, 0> { using type = double; };
template <typename A, typename T>
__device__ __forceinline__ A lq_fma(T x, T y, A acc) { return fma((A)x, (A)y, acc); }

// One thread per problem.  The sweep is a long chain of tiny dependent matrix products: straight from global
// memory every operand costs a ~600-cycle round trip (measured 720 us per call at B=1024, 2/1, H=20).  So a
// workgroup first copies the whole working set of its `ppw` problems (iterate, gradient, defects, tiles,
// Lagrangian blocks) into LDS with coalesced loads, the first ppw lanes then run their sweeps out of LDS
// (per-problem stride odd -> conflict-free), and the step / costates are copied back cooperatively.
// Problems whose working set does not fit in LDS fall back to global temporaries (ppw = 64, use_lds = 0).
// NX, NU > 0: dimensions fixed at compile time -- every small loop unrolls and the temporaries live in registers
// (2/1 and 6/3, the BASELINE shapes); NX = NU = 0: runtime dimensions, temporaries in LDS / global memory.
// SCAN (2/1 stages, LDS mode): the sweeps are replaced by lq_scan_problem, a wave per problem; staging and the post-pass
// are the same code.
template <typename T, int NX, int NU, bool LDS, bool SCAN = false>
__global__ __launch_bounds__(256) void solver_lq_kernel(SolverArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    T* lds = reinterpret_cast<T*>(lds_raw);
    const int lane = threadIdx.x;
    constexpr bool FIX = NX > 0;
    using Acc = typename LqAcc<T, NX>::type;
    const int H = a.H, nx = FIX ? NX : a.nx, nu = FIX ? NU : a.nu, nin = nx + nu, n = a.n;
    const int ppw = LDS ? a.ppw : 64;
    const int spec = LDS ? a.spec : 1;
    const int aj0 = lane < ppw * spec ? lane / ppw : 0;      // which of the side-by-side damping levels this lane sweeps
    const int pl = lane < ppw * spec ? lane - aj0 * ppw : lane;   // its problem's slot in the workgroup
    // element offsets of the per-problem LDS block: the arrays every attempt reads, the results, then one region per attempt
    const int Lz = 0, Lgr = Lz + n, Lgc = Lgr + n, Ltl = Lgc + H * nx, LW = Ltl + H * nx * nin, Llam = LW + H * nin * nin,
              Ldz = Llam + H * nx, Lbh = Ldz + n, Llc = Lbh + n, Lzl = Llc + H * nx, Lzu = Lzl + n,
              Latt = Lzu + n + aj0 * a.att_elems, LK = Latt, Lk = LK + H * nu * nx,
              LP = Lk + H * nu, Lp = LP + H * nx * nx, Ltmp = Lp + H * nx;
    const int b = blockIdx.x * ppw + pl;
    const bool mine = lane < ppw * spec && b < a.B;
    // cooperative staging, all four waves loading: a wave takes a problem (with fewer than three problems in the
    // workgroup, two or all four waves share one), its lanes the elements -- index arithmetic without divisions (a flat
    // index over problems x elements cost a ~40-instruction integer division per element, in a phase that a wave runs
    // once, at one instruction per ~10 cycles)
    const int b0 = blockIdx.x * ppw;
    const int np = a.B - b0 < ppw ? a.B - b0 : ppw;
    const int nthr = blockDim.x;
    const int wvu = __builtin_amdgcn_readfirstlane(lane >> 6);
    const int lgw = np >= 3 ? 0 : (np == 2 ? 1 : 2);                 // log2(waves per problem), 4 waves
    const int st_p0 = wvu >> lgw, st_pstep = 4 >> lgw, st_e0 = ((wvu & ((1 << lgw) - 1)) << 6) + (lane & 63), st_estep = 64 << lgw;
    // bounds (the same for every problem): one copy per workgroup behind the problem blocks; the post-pass reads them there
    T* const lds_lb = lds + (size_t)ppw * a.lds_stride;
    T* const lds_ub = lds_lb + n;
    auto stage_in = [&](const T* __restrict__ src, int per, int src_stride, int loff) {
        for (int pp = st_p0; pp < np; pp += st_pstep) {
            const T* sp = src + (size_t)(b0 + pp) * src_stride;
            T* dp = lds + (size_t)pp * a.lds_stride + loff;
            for (int e = st_e0; e < per; e += st_estep) dp[e] = sp[e];
        }
    };
    LQ_STAMP(0);
    if constexpr (LDS) {
        if (a.accept_first) {
            // acceptance test of the previous iteration's trial point for this workgroup's problems (a wave per problem), then
            // everything below reads the iterate it left: the staging waits behind the barrier
            for (int pp = wvu; pp < np; pp += 4)
                solver_merit_body<T>(a, (const T*)a.Zt_it, (const T*)a.gt_acc, (const T*)nullptr, (T*)a.Z, 2, (const int*)nullptr,
                                     (int*)nullptr, 1, b0 + pp, lane & 63, a.n_active_prev, a.cur_it);
            __syncthreads();
        }
    }
    // The scalars of the problem this wave solves (scan) and post-processes first -- status, damping, barrier parameter,
    // penalty, objective value, backtracking memory: requested with the staging loads, each was a ~2,000-cycle round trip of
    // its own where it is used (status before the solve, the others at the top of the post-pass)
    const int pf_b = b0 + wvu;
    const bool pf_ok = LDS && wvu < np;
    int pf_status = -1;
    T pf_reg = T(0), pf_mu = T(0), pf_pen = T(0), pf_f = T(0), pf_lsk = T(0), pf_lsa = T(0), pf_lsr = T(0);
    if (pf_ok) {
        pf_status = a.status[pf_b];
        pf_reg = ((const T*)a.reg)[pf_b];
        if (a.fuse_step) {
            const T* infp = (const T*)a.info + (size_t)pf_b * INFO_N;
            pf_mu = ((const T*)a.mu)[pf_b]; pf_pen = ((const T*)a.pen)[pf_b]; pf_f = ((const T*)a.f_it)[pf_b];
            pf_lsk = infp[INFO_LSK]; pf_lsa = infp[INFO_LSA]; pf_lsr = infp[INFO_LSR];
        }
    }
    if (LDS) {
        // counters of the convergence test (zeroed here unless the test runs inside this kernel: then the previous
        // iteration's acceptance kernel did it) and of the trial's acceptance test
        if (blockIdx.x == 0 && lane == 0) {
            if (a.fuse_step) *a.n_pending = 0; else *a.n_active = 0;
        }
        // Small stages (every array a few wavefuls: the BASELINE 2/1 shapes): ALL loads of a problem are issued before the
        // first LDS write, one global round trip instead of one per array and three inside the barrier terms
        const int Ntl = H * nx * nin, NW = H * nin * nin;
        const bool one_shot = n <= st_estep && Ntl <= 2 * st_estep && NW <= 3 * st_estep;
        if (one_shot) {
            for (int pp = st_p0; pp < np; pp += st_pstep) {
                const int bq = b0 + pp, e = st_e0, e1 = e + st_estep, e2 = e1 + st_estep;
                const bool in_n = e < n, pdl = a.primal_dual != 0;
                const T mu_q = ((const T*)a.mu)[bq];
                const int st_q = a.status[bq];
                const T vz = in_n ? ((const T*)a.Z)[(size_t)bq * n + e] : T(0);
                const T vgr = in_n ? ((const T*)a.grad)[(size_t)bq * n + e] : T(0);
                const T vlo = in_n ? solver_lb<T>(a, bq)[e] : -std::numeric_limits<T>::max();
                const T vhi = in_n ? solver_ub<T>(a, bq)[e] : std::numeric_limits<T>::max();
                const T vzl = in_n && pdl ? ((const T*)a.zl)[(size_t)bq * n + e] : T(0);
                const T vzu = in_n && pdl ? ((const T*)a.zu)[(size_t)bq * n + e] : T(0);
                const T vgc = e < H * nx ? ((const T*)a.g)[(size_t)bq * a.m + e] : T(0);
                const T vlc = e < H * nx && a.lam_t ? ((const T*)a.lam)[(size_t)bq * a.m + e] : T(0);
                const T* tq = (const T*)a.tiles + (size_t)bq * Ntl;
                const T* wq = (const T*)a.hblk + (size_t)bq * NW;
                const T vt0 = e < Ntl ? tq[e] : T(0), vt1 = e1 < Ntl ? tq[e1] : T(0);
                const T vw0 = e < NW ? wq[e] : T(0), vw1 = e1 < NW ? wq[e1] : T(0), vw2 = e2 < NW ? wq[e2] : T(0);
                T* blkp = lds + (size_t)pp * a.lds_stride;
                if (e < Ntl) blkp[Ltl + e] = vt0;
                if (e1 < Ntl) blkp[Ltl + e1] = vt1;
                if (e < NW) blkp[LW + e] = vw0;
                if (e1 < NW) blkp[LW + e1] = vw1;
                if (e2 < NW) blkp[LW + e2] = vw2;
                if (e < H * nx) { blkp[Lgc + e] = vgc; blkp[Llc + e] = vlc; }
                if (in_n) {
                    T ga, ha;
                    barrier_terms_of<T>(pdl, mu_q, st_q, vz, vlo, vhi, vzl, vzu, ga, ha);
                    blkp[Lz + e] = vz;
                    blkp[Lgr + e] = vgr + ga;
                    blkp[Lbh + e] = ha;
                    blkp[Lzl + e] = vzl; blkp[Lzu + e] = vzu;
                    // (every problem's stagers write the same values; per-problem bounds are read where they live)
                    if (!a.bstride) { lds_lb[e] = vlo; lds_ub[e] = vhi; }
                }
            }
            __syncthreads();
        } else {
        stage_in((const T*)a.Z, n, n, Lz);
        // gradient + barrier gradient, barrier diagonal: computed while staging (no solver_barrier_kernel launch)
        for (int pp = st_p0; pp < np; pp += st_pstep) {
            T* blkp = lds + (size_t)pp * a.lds_stride;
            for (int e = st_e0; e < n; e += st_estep) {
                T ga, ha;
                solver_barrier_terms<T>(a, b0 + pp, e, ga, ha);
                T gv = ((const T*)a.grad)[(size_t)(b0 + pp) * n + e];
                gv += ga;
                blkp[Lgr + e] = gv;
                blkp[Lbh + e] = ha;
            }
        }
        stage_in((const T*)a.g, H * nx, a.m, Lgc);
        if (a.primal_dual) { stage_in((const T*)a.zl, n, n, Lzl); stage_in((const T*)a.zu, n, n, Lzu); }
        if (!a.bstride)
            for (int e = lane; e < n; e += nthr) { lds_lb[e] = ((const T*)a.lb)[e]; lds_ub[e] = ((const T*)a.ub)[e]; }
        if (a.lam_t) stage_in((const T*)a.lam, H * nx, a.m, Llc);
        stage_in((const T*)a.tiles, H * nx * nin, H * nx * nin, Ltl);
        stage_in((const T*)a.hblk, H * nin * nin, H * nin * nin, LW);
        __syncthreads();
        }
    }
    LQ_STAMP(1);
    if constexpr (SCAN) {
        static_assert(LDS && NX == 2 && NU == 1, "the scan is written for 2-state / 1-control stages staged in LDS");
        for (int pp = wvu; pp < np; pp += 4)
            lq_scan_problem<T>(a, b0 + pp, lane & 63, lds + (size_t)pp * a.lds_stride, Lgr, Lgc, Ltl, LW, Llam, Ldz, Lbh,
                               pp == wvu ? pf_status : a.status[b0 + pp], pp == wvu ? pf_reg : ((const T*)a.reg)[b0 + pp]);
    } else {
    T* dzg = mine ? (T*)a.dz + (size_t)b * n : nullptr;
    if (mine && a.status[b] >= 0) {
        // finished problem: zero step (written through the copy-out below in LDS mode)
        if (aj0 == 0) {
            T* dzp = LDS ? lds + (size_t)pl * a.lds_stride + Ldz : dzg;
            for (int i = 0; i < n; ++i) dzp[i] = T(0);
            if (LDS) {
                T* lp = lds + (size_t)pl * a.lds_stride + Llam;
                const T* lcur = (const T*)a.lam + (size_t)b * a.m;
                for (int i = 0; i < H * nx; ++i) lp[i] = lcur[i];
            }
        }
    } else if (mine) {
    T* info = (T*)a.info + (size_t)b * INFO_N;
    T* blk = lds + (size_t)pl * a.lds_stride;
    T* tb = LDS ? blk + Ltmp : (T*)a.tmp + b;
    const size_t ts = LDS ? 1 : a.tmp_stride;
    T tmpv[FIX ? (3 * NX * NX + 3 * NX * NU + NU * NU + 5 * NX + 3 * NU) : 1];
#define TMP(e) (*(FIX ? &tmpv[FIX ? (e) : 0] : &tb[(size_t)(e) * ts]))
    int off = 0;
    const int oP = off; off += nx * nx;
    const int oPA = off; off += nx * nx;
    const int oPn = off; off += nx * nx;
    const int oPB = off; off += nx * nu;
    const int oQux = off; off += nu * nx;
    const int oK = off; off += nu * nx;
    const int oQuu = off; off += nu * nu;
    const int oPc = off; off += nx;
    const int op = off; off += nx;
    const int opn = off; off += nx;
    const int odx = off; off += nx;
    const int odxn = off; off += nx;
    const int oqu = off; off += nu;
    const int okv = off; off += nu;
    const int odu = off; off += nu;

    const T* z = LDS ? blk + Lz : (const T*)a.Z + (size_t)b * n;
    const T* gr = LDS ? blk + Lgr : (const T*)a.grad + (size_t)b * n;
    const T* gc = LDS ? blk + Lgc : (const T*)a.g + (size_t)b * a.m;
    const T* tl = LDS ? blk + Ltl : (const T*)a.tiles + (size_t)b * H * nx * nin;
    const T* Wb = LDS ? blk + LW : (const T*)a.hblk + (size_t)b * H * nin * nin;
    const T* Qs = (const T*)a.obj + a.oo.Qs;
    const T* QTs = (const T*)a.obj + a.oo.QTs;
    const T* Rs = (const T*)a.obj + a.oo.Rs;
    // small stages: the objective's weights live in registers for the sweeps (read from global memory inside the stage
    // loop they were two ~500-cycle waits per stage: the stores of the sweep keep the compiler from hoisting them)
    constexpr bool REGTAB = FIX && NX * NX + NU * NU <= 16;
    T Qr[REGTAB ? NX * NX : 1], Rr[REGTAB ? NU * NU : 1];
    if (REGTAB) {
        #pragma unroll
        for (int e = 0; e < NX * NX; ++e) Qr[REGTAB ? e : 0] = Qs[e];
        #pragma unroll
        for (int e = 0; e < NU * NU; ++e) Rr[REGTAB ? e : 0] = Rs[e];
    }
#define QS(e) (REGTAB ? Qr[REGTAB ? (e) : 0] : Qs[e])
#define RS(e) (REGTAB ? Rr[REGTAB ? (e) : 0] : Rs[e])
    const T* lb = solver_lb<T>(a, b);
    const T* ub = solver_ub<T>(a, b);
    const T* bh = LDS ? blk + Lbh : (const T*)a.bh + (size_t)b * n;   // barrier diagonal (solver_barrier_kernel)
    T reg = ((const T*)a.reg)[b];
    T* Kst = LDS ? blk + LK : (T*)a.Kst + (size_t)b * H * nu * nx;
    T* kst = LDS ? blk + Lk : (T*)a.kst + (size_t)b * H * nu;
    T* Pst = LDS ? blk + LP : (T*)a.Pst + (size_t)b * H * nx * nx;
    T* pst = LDS ? blk + Lp : (T*)a.pst + (size_t)b * H * nx;
    T* dz = LDS ? blk + Ldz : dzg;
    const int uo = H * nx;

    // Damping levels side by side: a sweep that meets an indefinite pivot has to be repeated with more damping, and the
    // launch waited for the problem in hundreds that needs the third attempt (one sweep is a ~20 us latency chain of one
    // lane; the levels are known beforehand: half-decade steps).  `spec` lanes per problem now run the levels of a round at the
    // same time, each into its own region of the problem's block; the FIRST level that goes through is the one used, so
    // the result is what the sequential attempts gave.
    constexpr bool PREF = FIX && NX * (NX + NU) + (NX + NU) * (NX + NU) <= 16;
    struct StageIn {
        T At[PREF ? NX * (NX + NU) : 1], W[PREF ? (NX + NU) * (NX + NU) : 1], gc[PREF ? NX : 1], gru[PREF ? NU : 1],
            bhu[PREF ? NU : 1], grx[PREF ? NX : 1], bhx[PREF ? NX : 1];
    };
    auto fetch_stage = [&](const int t, StageIn& d) {
        #pragma unroll
        for (int e = 0; e < nx * nin; ++e) d.At[PREF ? e : 0] = tl[(size_t)t * nx * nin + e];
        #pragma unroll
        for (int e = 0; e < nin * nin; ++e) d.W[PREF ? e : 0] = Wb[(size_t)t * nin * nin + e];
        #pragma unroll
        for (int i = 0; i < nx; ++i) d.gc[PREF ? i : 0] = gc[t * nx + i];
        #pragma unroll
        for (int i = 0; i < nu; ++i) { d.gru[PREF ? i : 0] = gr[uo + t * nu + i]; d.bhu[PREF ? i : 0] = bh[uo + t * nu + i]; }
        if (t > 0) {
            #pragma unroll
            for (int i = 0; i < nx; ++i) { d.grx[PREF ? i : 0] = gr[(t - 1) * nx + i]; d.bhx[PREF ? i : 0] = bh[(t - 1) * nx + i]; }
        }
    };
#define AT(e) (PREF ? cur.At[PREF ? (e) : 0] : At[e])
#define WT(e) (PREF ? cur.W[PREF ? (e) : 0] : Wt[e])
#define GC(k) (PREF ? cur.gc[PREF ? (k) : 0] : gc[t * nx + (k)])
#define GRU(i) (PREF ? cur.gru[PREF ? (i) : 0] : gr[uo + t * nu + (i)])
#define BHU(i) (PREF ? cur.bhu[PREF ? (i) : 0] : bh[uo + t * nu + (i)])
#define GRX(i) (PREF ? cur.grx[PREF ? (i) : 0] : gr[(t - 1) * nx + (i)])
#define BHX(i) (PREF ? cur.bhx[PREF ? (i) : 0] : bh[(t - 1) * nx + (i)])
    StageIn sin_a, sin_b;
    int restarts = 0;
    bool solved = false, any = false;
    const T reg_in = reg;
    for (int base = 0; base < a.lq_attempts && !any; base += spec) {
    const int aj = base + aj0;
    reg = reg_in;
    for (int k = 0; k < aj; ++k) reg = fmax(reg * (T)a.reg_raise, T(NEMPC_REG_FLOOR));
    bool pd = aj < a.lq_attempts;
    // terminal value function: V_{H-1}(dx) = 1/2 dx' Hx dx + gx' dx
    #pragma unroll
    for (int i = 0; i < nx; ++i) {
        T ga = T(0), ha = T(0);
        ha = bh[(H - 1) * nx + i];
        #pragma unroll
        for (int j = 0; j < nx; ++j) TMP(oP + i * nx + j) = QTs[i * nx + j] + (i == j ? ha : T(0));   // terminal weight
        TMP(op + i) = gr[(H - 1) * nx + i];
    }
    if (PREF && pd) fetch_stage(H - 1, sin_a);
    // One stage of the backward recursion.  Small stages (2/1): the stage's inputs (tile, Lagrangian block, defects,
    // gradient and barrier entries) come from registers that were loaded a whole stage earlier (`cur`), and the next
    // stage's are requested at the top (`nxt`) -- the sweep no longer stops four or five times per stage for an LDS
    // round trip behind the stores of the recursion, which the compiler must assume to alias the loads.
    auto stage = [&](const int t, const StageIn& cur, StageIn& nxt) -> bool {
        if (PREF && t > 0) fetch_stage(t - 1, nxt);
        const T* At = tl + (size_t)t * nx * nin;   // [i][0:nx] = A, [i][nx:] = B
        const T* Wt = Wb + (size_t)t * nin * nin;  // Lagrangian block over (x_{t-1}, u_t)
        #pragma unroll
        for (int i = 0; i < nx; ++i) {
            #pragma unroll
            for (int j = 0; j < nx; ++j) Pst[(size_t)t * nx * nx + i * nx + j] = TMP(oP + i * nx + j);
            pst[(size_t)t * nx + i] = TMP(op + i);
        }
        // PA = P A, PB = P B, Pc = P c + p
        #pragma unroll
        for (int i = 0; i < nx; ++i) {
            if (t > 0 || FIX)     // (fixed shapes: unconditional -- a guard turns into a select per entry and stage)
                #pragma unroll
                for (int j = 0; j < nx; ++j) {
                    Acc v_acc = T(0);
                    #pragma unroll
                    for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(TMP(oP + i * nx + k), AT(k * nin + j), v_acc);
                    const T v = (T)v_acc;
                    TMP(oPA + i * nx + j) = v;
                }
            #pragma unroll
            for (int j = 0; j < nu; ++j) {
                Acc v_acc = T(0);
                #pragma unroll
                for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(TMP(oP + i * nx + k), AT(k * nin + nx + j), v_acc);
                const T v = (T)v_acc;
                TMP(oPB + i * nu + j) = v;
            }
            Acc v_acc = TMP(op + i);
            #pragma unroll
            for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(TMP(oP + i * nx + k), GC(k), v_acc);
            const T v = (T)v_acc;
            TMP(oPc + i) = v;
        }
        // Quu = Rs + barrier + reg + B' PB ; qu = gu + barrier + B' Pc ; Qux = B' PA
        #pragma unroll
        for (int i = 0; i < nu; ++i) {
            T ga = T(0), ha = T(0);
            ha = BHU(i);
            #pragma unroll
            for (int j = 0; j < nu; ++j) {
                Acc v_acc = RS(i * nu + j) + WT((nx + i) * nin + nx + j) + (i == j ? ha + reg : T(0));
                #pragma unroll
                for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(AT(k * nin + nx + i), TMP(oPB + k * nu + j), v_acc);
                const T v = (T)v_acc;
                TMP(oQuu + i * nu + j) = v;
            }
            Acc v_acc = GRU(i);
            #pragma unroll
            for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(AT(k * nin + nx + i), TMP(oPc + k), v_acc);
            const T v = (T)v_acc;
            TMP(oqu + i) = v;
            if (t > 0 || FIX)     // (fixed shapes: unconditional -- a guard turns into a select per entry and stage)
                #pragma unroll
                for (int j = 0; j < nx; ++j) {
                    Acc w_acc = WT((nx + i) * nin + j);
                    #pragma unroll
                    for (int k = 0; k < nx; ++k) w_acc = lq_fma<Acc>(AT(k * nin + nx + i), TMP(oPA + k * nx + j), w_acc);
                    const T w = (T)w_acc;
                    TMP(oQux + i * nx + j) = w;
                }
        }
        // Cholesky Quu = L L' (lower, in place)
        #pragma unroll
        for (int j = 0; j < nu; ++j) {
            T d = TMP(oQuu + j * nu + j);
            #pragma unroll
            for (int k = 0; k < j; ++k) d -= TMP(oQuu + j * nu + k) * TMP(oQuu + j * nu + k);
            if (!(d > T(1e-12))) { pd = false; break; }   // not positive definite: restart with more damping
            // the diagonal of L is only ever divided by: its INVERSE is kept in its place (one division per pivot instead
            // of one per use -- seven per stage at 2/1 -- in a sweep whose time is its instruction count)
            d = inv_sqrt_pos(d);
            TMP(oQuu + j * nu + j) = d;
            #pragma unroll
            for (int i = j + 1; i < nu; ++i) {
                T v = TMP(oQuu + i * nu + j);
                #pragma unroll
                for (int k = 0; k < j; ++k) v -= TMP(oQuu + i * nu + k) * TMP(oQuu + j * nu + k);
                TMP(oQuu + i * nu + j) = v * d;
            }
        }
        if (!pd) return false;
        // kv = -Quu^-1 qu ; K = -Quu^-1 Qux   (forward then backward substitution, column by column)
        const int ncolK = t > 0 || FIX ? nx : 0;
        for (int col = -1; col < ncolK; ++col) {
            #pragma unroll
            for (int i = 0; i < nu; ++i) {
                T v = (col < 0) ? TMP(oqu + i) : TMP(oQux + i * nx + col);
                #pragma unroll
                for (int k = 0; k < i; ++k) v -= TMP(oQuu + i * nu + k) * TMP(odu + k);
                TMP(odu + i) = v * TMP(oQuu + i * nu + i);
            }
            #pragma unroll
            for (int i = nu - 1; i >= 0; --i) {
                T v = TMP(odu + i);
                #pragma unroll
                for (int k = i + 1; k < nu; ++k) v -= TMP(oQuu + k * nu + i) * TMP(odu + k);
                v *= TMP(oQuu + i * nu + i);
                TMP(odu + i) = v;
            }
            #pragma unroll
            for (int i = 0; i < nu; ++i) {
                if (col < 0) { TMP(okv + i) = -TMP(odu + i); kst[(size_t)t * nu + i] = -TMP(odu + i); }
                else { TMP(oK + i * nx + col) = -TMP(odu + i); Kst[(size_t)t * nu * nx + i * nx + col] = -TMP(odu + i); }
            }
        }
        if (t > 0) {
            // P_{t-1} = Hx_{t-1} + A' PA + Qux' K ; p_{t-1} = gx_{t-1} + A' Pc + Qux' kv
            #pragma unroll
            for (int i = 0; i < nx; ++i) {
                T ga = T(0), ha = T(0);
                ha = BHX(i);
                #pragma unroll
                for (int j = 0; j < nx; ++j) {
                    Acc v_acc = QS(i * nx + j) + WT(i * nin + j) + (i == j ? ha : T(0));
                    #pragma unroll
                    for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(AT(k * nin + i), TMP(oPA + k * nx + j), v_acc);
                    #pragma unroll
                    for (int k = 0; k < nu; ++k) v_acc = lq_fma<Acc>(TMP(oQux + k * nx + i), TMP(oK + k * nx + j), v_acc);
                    const T v = (T)v_acc;
                    TMP(oPn + i * nx + j) = v;
                }
                Acc v_acc = GRX(i);
                #pragma unroll
                for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(AT(k * nin + i), TMP(oPc + k), v_acc);
                #pragma unroll
                for (int k = 0; k < nu; ++k) v_acc = lq_fma<Acc>(TMP(oQux + k * nx + i), TMP(okv + k), v_acc);
                const T v = (T)v_acc;
                TMP(opn + i) = v;
            }
            #pragma unroll
            for (int i = 0; i < nx; ++i) {
                #pragma unroll
                for (int j = 0; j < nx; ++j)
                    TMP(oP + i * nx + j) = i == j ? TMP(oPn + i * nx + j) : T(0.5) * (TMP(oPn + i * nx + j) + TMP(oPn + j * nx + i));
                TMP(op + i) = TMP(opn + i);
            }
        }
            return true;
    };
    for (int t = H - 1; t >= 0 && pd; t -= 2) {
        pd = stage(t, sin_a, sin_b);
        if (pd && t > 0) pd = stage(t - 1, sin_b, sin_a);
    }
    {
        const unsigned long long ok = __ballot(pd);
        int win = -1;
        for (int jj = spec - 1; jj >= 0; --jj)
            if ((ok >> (jj * ppw + pl)) & 1ull) win = jj;
        if (win >= 0) { any = true; solved = win == aj0; restarts = base + win; }
    }
    // half-decade steps (reg_raise = sqrt(10); the attempt counts below are whole-decade ones: 1e-3 .. 100 in six) from a floor
    // of 1e-3: whenever a sweep of this problem family fails, the damping that lets it through
    // is 0.1 .. 100 (NEMPC_SOLVER_STATS), and the whole launch waits for the one problem in hundreds that climbs there --
    // nine attempts from the relaxed value with a floor of 1e-6, six from 1e-3 (the kernel runs 37 us clean, 10 us more
    // per attempt).  Remembering per problem the level that worked last time did not help: the restarting problems are
    // mostly first-timers.
    }
    if (!any) {
        restarts = a.lq_attempts;
        reg = reg_in;
        for (int k = 0; k < a.lq_attempts; ++k) reg = fmax(reg * (T)a.reg_raise, T(NEMPC_REG_FLOOR));
    }
    if (solved || (!any && aj0 == 0)) ((T*)a.reg)[b] = reg;
    T* lamn = LDS ? blk + Llam : (T*)a.lamn + (size_t)b * a.m;
    if (!solved && (any || aj0 != 0)) {
        // another lane of this problem holds the level that is used (or reports that none went through)
    } else if (!solved) {
        // Out of attempts for this iteration.  The launch waits for its slowest problem, and the one problem in hundreds
        // that needs five or six decades of damping made every other one wait ~50 us for it: it now keeps the damping it
        // has climbed to, takes NO step this iteration (zero step, multipliers unchanged, marked by a negative restart
        // count) and goes on climbing in the next one.
        for (int i = 0; i < n; ++i) dz[i] = T(0);
        const T* lcur = (const T*)a.lam + (size_t)b * a.m;
        for (int i = 0; i < H * nx; ++i) lamn[i] = lcur[i];
        info[INFO_STEP] = std::numeric_limits<T>::max();
        info[INFO_RESTARTS] = (T)(-restarts);
        if (LDS) blk[Lbh] = (T)(-restarts);          // (the barrier diagonal is no longer needed: slot for the post-pass)
    } else {
    LQ_STAMP(9);
    // forward sweep
    // The norms, the directional derivative and the fraction-to-the-boundary length of the step are NOT part of the
    // recursion: in LDS mode a wave per problem computes them from the staged arrays after the sweeps (below), with its
    // 64 lanes over the elements -- in the sweep they were 60 % of the forward pass's instructions (three divisions per
    // stage among them), issued one per ~10 cycles by a lone lane (kernel 37 -> 22 us clean)
    const bool norms_here = !LDS;
    T lam_inf = T(0), step_inf = T(0), amax = T(1), D0 = T(0), g1 = T(0), ginf = T(0), zinf = T(0);
    const T tau = T(0.995);
    #pragma unroll
    for (int i = 0; i < nx; ++i) TMP(odx + i) = T(0);
    if (PREF && LDS) {
        // small stages: as in the backward sweep, a stage's inputs (gains, tile, defects, value function) are in registers,
        // requested one stage ahead -- the recursion carries dx only, and no longer stops twice per stage for LDS round
        // trips behind its own stores
        struct FwdIn {
            T k[PREF ? NU : 1], K[PREF ? NU * NX : 1], A[PREF ? NX * (NX + NU) : 1], gc[PREF ? NX : 1], P[PREF ? NX * NX : 1],
                p[PREF ? NX : 1];
        };
        auto fetch_f = [&](const int t, FwdIn& d) {
            #pragma unroll
            for (int e = 0; e < nu; ++e) d.k[PREF ? e : 0] = kst[(size_t)t * nu + e];
            #pragma unroll
            for (int e = 0; e < nu * nx; ++e) d.K[PREF ? e : 0] = Kst[(size_t)t * nu * nx + e];
            #pragma unroll
            for (int e = 0; e < nx * nin; ++e) d.A[PREF ? e : 0] = tl[(size_t)t * nx * nin + e];
            #pragma unroll
            for (int e = 0; e < nx; ++e) { d.gc[PREF ? e : 0] = gc[t * nx + e]; d.p[PREF ? e : 0] = pst[(size_t)t * nx + e]; }
            #pragma unroll
            for (int e = 0; e < nx * nx; ++e) d.P[PREF ? e : 0] = Pst[(size_t)t * nx * nx + e];
        };
        auto fstage = [&](const int t, const FwdIn& c, FwdIn& nxt) {
            if (t + 1 < H) fetch_f(t + 1, nxt);
            #pragma unroll
            for (int i = 0; i < nu; ++i) {
                T v = c.k[PREF ? i : 0];
                if (t > 0)
                    #pragma unroll
                    for (int k = 0; k < nx; ++k) v = fma(c.K[PREF ? i * nx + k : 0], TMP(odx + k), v);
                TMP(odu + i) = v;
            }
            #pragma unroll
            for (int i = 0; i < nx; ++i) {
                T v = c.gc[PREF ? i : 0];
                if (t > 0)
                    #pragma unroll
                    for (int k = 0; k < nx; ++k) v = fma(c.A[PREF ? i * nin + k : 0], TMP(odx + k), v);
                #pragma unroll
                for (int k = 0; k < nu; ++k) v = fma(c.A[PREF ? i * nin + nx + k : 0], TMP(odu + k), v);
                TMP(odxn + i) = v;
            }
            #pragma unroll
            for (int i = 0; i < nx; ++i) {
                T lam = c.p[PREF ? i : 0];
                #pragma unroll
                for (int k = 0; k < nx; ++k) lam = fma(c.P[PREF ? i * nx + k : 0], TMP(odxn + k), lam);
                lamn[t * nx + i] = lam;
                dz[t * nx + i] = TMP(odxn + i);
            }
            #pragma unroll
            for (int i = 0; i < nx; ++i) TMP(odx + i) = TMP(odxn + i);
            #pragma unroll
            for (int i = 0; i < nu; ++i) dz[uo + t * nu + i] = TMP(odu + i);
        };
        FwdIn fa, fb;
        fetch_f(0, fa);
        for (int t = 0; t < H; t += 2) {
            fstage(t, fa, fb);
            if (t + 1 < H) fstage(t + 1, fb, fa);
        }
    } else
    for (int t = 0; t < H; ++t) {
        const T* At = tl + (size_t)t * nx * nin;
        #pragma unroll
        for (int i = 0; i < nu; ++i) {
            Acc v_acc = kst[(size_t)t * nu + i];
            if (t > 0)
                #pragma unroll
                for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(Kst[(size_t)t * nu * nx + i * nx + k], TMP(odx + k), v_acc);
            const T v = (T)v_acc;
            TMP(odu + i) = v;
        }
        #pragma unroll
        for (int i = 0; i < nx; ++i) {
            Acc v_acc = gc[t * nx + i];
            if (t > 0)
                #pragma unroll
                for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(At[i * nin + k], TMP(odx + k), v_acc);
            #pragma unroll
            for (int k = 0; k < nu; ++k) v_acc = lq_fma<Acc>(At[i * nin + nx + k], TMP(odu + k), v_acc);
            const T v = (T)v_acc;
            TMP(odxn + i) = v;
        }
        #pragma unroll
        for (int i = 0; i < nx; ++i) {
            Acc lam_acc = pst[(size_t)t * nx + i];
            #pragma unroll
            for (int k = 0; k < nx; ++k) lam_acc = lq_fma<Acc>(Pst[(size_t)t * nx * nx + i * nx + k], TMP(odxn + k), lam_acc);
            const T lam = (T)lam_acc;
            lamn[t * nx + i] = lam;
            const T d = TMP(odxn + i);
            dz[t * nx + i] = d;
            TMP(odx + i) = d;
            if (norms_here) {
                const T zz = z[t * nx + i], lo = lb[t * nx + i], hi = ub[t * nx + i];
                lam_inf = fmax(lam_inf, fabs(lam));
                step_inf = fmax(step_inf, fabs(d));
                zinf = fmax(zinf, fabs(zz));
                D0 = fma(gr[t * nx + i], d, D0);
                if (d < T(0) && lo > -std::numeric_limits<T>::max()) amax = fmin(amax, tau * (zz - lo) / (-d));
                if (d > T(0) && hi < std::numeric_limits<T>::max()) amax = fmin(amax, tau * (hi - zz) / d);
                const T gv = fabs(gc[t * nx + i]);
                g1 += gv;
                ginf = fmax(ginf, gv);
            }
        }
        #pragma unroll
        for (int i = 0; i < nu; ++i) {
            const T d = TMP(odu + i);
            dz[uo + t * nu + i] = d;
            if (norms_here) {
                const T zz = z[uo + t * nu + i], lo = lb[uo + t * nu + i], hi = ub[uo + t * nu + i];
                step_inf = fmax(step_inf, fabs(d));
                zinf = fmax(zinf, fabs(zz));
                D0 = fma(gr[uo + t * nu + i], d, D0);
                if (d < T(0) && lo > -std::numeric_limits<T>::max()) amax = fmin(amax, tau * (zz - lo) / (-d));
                if (d > T(0) && hi < std::numeric_limits<T>::max()) amax = fmin(amax, tau * (hi - zz) / d);
            }
        }
    }
    if (norms_here) {
        info[INFO_LAM] = lam_inf; info[INFO_STEP] = step_inf; info[INFO_AMAX] = amax; info[INFO_G1] = g1;
        info[INFO_GINF] = ginf; info[INFO_D0] = D0; info[INFO_ZINF] = zinf;
    }
    info[INFO_RESTARTS] = (T)restarts;
    if (LDS) blk[Lbh] = (T)restarts;
    }   // solved
#undef TMP
#undef QS
#undef RS
#undef AT
#undef WT
#undef GC
#undef GRU
#undef BHU
#undef GRX
#undef BHX
    }
    }   // !SCAN
    LQ_STAMP(2);
    if (LDS) {
        __syncthreads();
        LQ_STAMP(3);
        {
            // norms of the steps just computed: wave w takes problems w, w + #waves, ...
            const int wv = lane >> 6, ln = lane & 63, nwv = nthr >> 6;
            const T tau = T(0.995);
            for (int pp = wv; pp < np; pp += nwv) {
                const int bp = b0 + pp;
                // the workgroup's LDS copy of the shared bounds, or this problem's own row in global memory
                const T* lb = a.bstride ? solver_lb<T>(a, bp) : lds_lb;
                const T* ub = a.bstride ? solver_ub<T>(a, bp) : lds_ub;
                const T* blk = lds + (size_t)pp * a.lds_stride;
                // the problem's scalars for the step part below: all requested now, used after the norms
                const T* infg = (const T*)a.info + (size_t)bp * INFO_N;
                StepInfo<T> si;
                if (pp == wvu && pf_ok) {       // (nothing in this kernel has written them since the prefetch)
                    si.status = pf_status;
                    si.mu = pf_mu; si.nu = pf_pen; si.f = pf_f; si.lsk = pf_lsk; si.lsa = pf_lsa; si.lsr = pf_lsr;
                } else {
                    si.status = a.status[bp];
                    if (a.fuse_step) {
                        si.mu = ((const T*)a.mu)[bp]; si.nu = ((const T*)a.pen)[bp]; si.f = ((const T*)a.f_it)[bp];
                        si.lsk = infg[INFO_LSK]; si.lsa = infg[INFO_LSA]; si.lsr = infg[INFO_LSR];
                    }
                }
                if (si.status >= 0) {
                    if (a.fuse_step) {      // finished problem: no step, its trial point is the iterate
                        if (ln == 0) a.lsdone[bp] = 1;
                        T* zt = (T*)a.Zt_it + (size_t)bp * n;
                        for (int i = ln; i < n; i += 64) zt[i] = blk[Lz + i];
                    }
                    continue;
                }
                T lam_inf = T(0), step_inf = T(0), amax = T(1), D0 = T(0), g1 = T(0), ginf = T(0), zinf = T(0);
                for (int i = ln; i < n; i += 64) {
                    const T d = blk[Ldz + i], zz = blk[Lz + i], lo = lb[i], hi = ub[i];
                    step_inf = fmax(step_inf, fabs(d));
                    zinf = fmax(zinf, fabs(zz));
                    D0 = fma(blk[Lgr + i], d, D0);
                    if (d < T(0) && lo > -std::numeric_limits<T>::max()) amax = fmin(amax, tau * (zz - lo) / (-d));
                    if (d > T(0) && hi < std::numeric_limits<T>::max()) amax = fmin(amax, tau * (hi - zz) / d);
                }
                for (int i = ln; i < H * nx; i += 64) {
                    lam_inf = fmax(lam_inf, fabs(blk[Llam + i]));
                    const T gv = fabs(blk[Lgc + i]);
                    g1 += gv;
                    ginf = fmax(ginf, gv);
                }
                // (on the vector unit alone: each shuffle tree was six dependent LDS round trips of a lone wave)
                lam_inf = (T)wave_max_lane0((double)lam_inf);
                step_inf = (T)wave_max_lane0((double)step_inf);
                amax = (T)wave_min_lane0((double)amax);
                D0 = (T)wave_sum_lane0((double)D0);
                g1 = (T)wave_sum_lane0((double)g1);
                ginf = (T)wave_max_lane0((double)ginf);
                zinf = (T)wave_max_lane0((double)zinf);
                LQ_STAMP(4);
                const T rst = blk[Lbh];                    // restart count left by the sweeping lane (negative: sat out)
                const bool sat_out = rst < T(0);           // no step this iteration: keep the sentinel
                if (ln == 0) {
                    T* info = (T*)a.info + (size_t)bp * INFO_N;
                    info[INFO_LAM] = lam_inf; info[INFO_STEP] = sat_out ? std::numeric_limits<T>::max() : step_inf;
                    info[INFO_AMAX] = amax; info[INFO_G1] = g1;
                    info[INFO_GINF] = ginf; info[INFO_D0] = D0; info[INFO_ZINF] = zinf;
                }
                if (a.fuse_step) {
                    // what solver_step_kernel does, from the LDS copies and the norms still in registers: dual steps of the
                    // bounds, convergence test / barrier update / merit at the iterate, first trial point
                    si.ginf = (T)wave_bcast_lane0((double)ginf); si.zinf = (T)wave_bcast_lane0((double)zinf);
                    si.lam = (T)wave_bcast_lane0((double)lam_inf);
                    si.d0 = (T)wave_bcast_lane0((double)D0); si.amax = (T)wave_bcast_lane0((double)amax);
                    si.step = sat_out ? std::numeric_limits<T>::max() : (T)wave_bcast_lane0((double)step_inf);
                    si.restarts = rst;
                    solver_dual_body<T>(a, bp, ln, blk + Lz, blk + Ldz, si.mu, si.status, lb, ub, blk + Lzl, blk + Lzu);
                    LQ_STAMP(5);
                    int lsd;
                    T al;
                    solver_merit0_body<T>(a, bp, ln, (const T*)a.f_it, blk + Lz, blk + Lgc, si, lsd, al, lb, ub);
                    LQ_STAMP(6);
                    T* zt = (T*)a.Zt_it + (size_t)bp * n;
                    for (int i = ln; i < n; i += 64) zt[i] = lsd ? blk[Lz + i] : fma(al, blk[Ldz + i], blk[Lz + i]);
                    if (a.lam_t) {       // multipliers of the trial point (what the acceptance kernel sets on acceptance)
                        T* lt = (T*)a.lam_t + (size_t)bp * a.m;
                        for (int i = ln; i < H * nx; i += 64) {
                            const T l0 = blk[Llc + i];          // (the current multipliers were staged with the working set)
                            lt[i] = lsd ? l0 : fma(al, blk[Llam + i] - l0, l0);
                        }
                    }
                }
            }
        }
        LQ_STAMP(7);
        auto stage_out = [&](T* __restrict__ dst, int per, int dst_stride, int loff) {
            for (int pp = st_p0; pp < np; pp += st_pstep) {
                T* dp = dst + (size_t)(b0 + pp) * dst_stride;
                const T* sp = lds + (size_t)pp * a.lds_stride + loff;
                for (int e = st_e0; e < per; e += st_estep) dp[e] = sp[e];
            }
        };
        stage_out((T*)a.dz, n, n, Ldz);
        stage_out((T*)a.lamn, H * nx, a.m, Llam);
    }
    LQ_STAMP(8);
}

}  // namespace

}  // namespace nempc
