// Batched solver, LQ solve by a Riccati sweep with a wave per problem (LDS mode).  Included by solver.hip only, after
// solver_lq_impl.h (inv_sqrt_pos).
#pragma once

namespace nempc {

namespace {

// Wave-per-problem variant of the LQ solve (LDS mode only): the same recursion, formulas and summation order as
// solver_lq_kernel, but every small matrix operation of a stage is spread over the 64 lanes of the problem's wave
// (entry per lane) with wave-level synchronisation between dependent operations.  A thread-per-problem sweep is one
// serial chain of ~1000 FMAs per stage on 6/3-sized blocks with 4 of 64 lanes busy; here a stage is ~8 short phases.
// NX, NU > 0: stage dimensions fixed at compile time (the entry loops unroll and their LDS loads overlap).
template <typename T, int NX, int NU>
__global__ __launch_bounds__(256) void solver_lqw_kernel(SolverArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    using Acc = typename LqAcc<T, NX>::type;       // (the sums' accumulator: solver_lq_impl.h)
    T* lds = reinterpret_cast<T*>(lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int H = a.H, nx = NX > 0 ? NX : a.nx, nu = NX > 0 ? NU : a.nu, nin = nx + nu, n = a.n;
    const int ppw = a.ppw;                       // == waves per workgroup
    const int b0 = blockIdx.x * ppw;
    const int np = a.B - b0 < ppw ? a.B - b0 : ppw;
    const int Lz = 0, Lgr = Lz + n, Lgc = Lgr + n, Ltl = Lgc + H * nx, LW = Ltl + H * nx * nin, Llam = LW + H * nin * nin,
              Ldz = Llam + H * nx, Lbh = Ldz + n, LK = Lbh + n, Lk = LK + H * nu * nx, LP = Lk + H * nu, Lp = LP + H * nx * nx,
              Ltmp = Lp + H * nx;
    auto stage_in = [&](const T* __restrict__ src, int per, int src_stride, int loff) {
        const int tot = np * per;
        const T* base = src + (size_t)b0 * src_stride;
        for (int i = tid; i < tot; i += 256) {
            const int pp = i / per, e = i - pp * per;
            lds[(size_t)pp * a.lds_stride + loff + e] = base[(size_t)pp * src_stride + e];
        }
    };
    if (blockIdx.x == 0 && tid == 0) *a.n_active = 0;       // counter of the convergence test that follows this kernel
    stage_in((const T*)a.Z, n, n, Lz);
    for (int i = tid; i < np * n; i += 256) {               // gradient + barrier gradient, barrier diagonal
        const int pp = i / n, e = i - pp * n;
        T ga, ha;
        solver_barrier_terms<T>(a, b0 + pp, e, ga, ha);
        T* blkp = lds + (size_t)pp * a.lds_stride;
        T gv = ((const T*)a.grad)[(size_t)(b0 + pp) * n + e];
        gv += ga;
        blkp[Lgr + e] = gv;
        blkp[Lbh + e] = ha;
    }
    stage_in((const T*)a.g, H * nx, a.m, Lgc);
    stage_in((const T*)a.tiles, H * nx * nin, H * nx * nin, Ltl);
    stage_in((const T*)a.hblk, H * nin * nin, H * nin * nin, LW);
    __syncthreads();

    const int b = b0 + wv;
    if (wv < np) {
        T* blk = lds + (size_t)wv * a.lds_stride;
        auto wsync = [] {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
        if (a.status[b] >= 0) {
            // finished problem: zero step, multipliers unchanged
            for (int i = lane; i < n; i += 64) blk[Ldz + i] = T(0);
            const T* lcur = (const T*)a.lam + (size_t)b * a.m;
            for (int i = lane; i < H * nx; i += 64) blk[Llam + i] = lcur[i];
        } else {
            T* tb = blk + Ltmp;
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
            const int oflag = off;                 // 1 slot: Cholesky verdict of the stage
            const T* z = blk + Lz;
            const T* gr = blk + Lgr;
            const T* gc = blk + Lgc;
            const T* tl = blk + Ltl;
            const T* Wb = blk + LW;
            const T* Qs = (const T*)a.obj + a.oo.Qs;
            const T* QTs = (const T*)a.obj + a.oo.QTs;
            const T* Rs = (const T*)a.obj + a.oo.Rs;
            const T* lb = solver_lb<T>(a, b);
            const T* ub = solver_ub<T>(a, b);
            const T* bh = blk + Lbh;                                             // barrier diagonal (solver_barrier_kernel)
            T reg = ((const T*)a.reg)[b];
            T* Kst = blk + LK;
            T* kst = blk + Lk;
            T* Pst = blk + LP;
            T* pst = blk + Lp;
            T* dz = blk + Ldz;
            T* lamn = blk + Llam;
            const int uo = H * nx;
            int restarts = 0;
            bool solved = false;
            for (int attempt = 0; attempt < a.lq_attempts; ++attempt) {
                bool pd = true;
                // terminal value function
                for (int e = lane; e < nx * nx + nx; e += 64) {
                    if (e < nx * nx) {
                        const int i = e / nx, j = e - i * nx;
                        T ga = T(0), ha = T(0);
                        if (i == j) ha = bh[(H - 1) * nx + i];
                        tb[oP + e] = QTs[e] + (i == j ? ha : T(0));   // terminal weight
                    } else {
                        const int i = e - nx * nx;
                        T ga = T(0), ha = T(0);
                        ha = bh[(H - 1) * nx + i];
                        tb[op + i] = gr[(H - 1) * nx + i] + ga;
                    }
                }
                wsync();
                for (int t = H - 1; t >= 0 && pd; --t) {
                    const T* At = tl + (size_t)t * nx * nin;
                    const T* Wt = Wb + (size_t)t * nin * nin;
                    // store P_t, p_t; PA = P A, PB = P B, Pc = P c + p
                    for (int e = lane; e < 2 * nx * nx + nx * nu + 2 * nx; e += 64) {
                        int r = e;
                        if (r < nx * nx) { Pst[(size_t)t * nx * nx + r] = tb[oP + r]; continue; }
                        r -= nx * nx;
                        if (r < nx) { pst[(size_t)t * nx + r] = tb[op + r]; continue; }
                        r -= nx;
                        if (r < nx * nx) {
                            if (t > 0) {
                                const int i = r / nx, j = r - i * nx;
                                Acc v_acc = T(0);
                                for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(tb[oP + i * nx + k], At[k * nin + j], v_acc);
                                const T v = (T)v_acc;
                                tb[oPA + r] = v;
                            }
                            continue;
                        }
                        r -= nx * nx;
                        if (r < nx * nu) {
                            const int i = r / nu, j = r - i * nu;
                            Acc v_acc = T(0);
                            for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(tb[oP + i * nx + k], At[k * nin + nx + j], v_acc);
                            const T v = (T)v_acc;
                            tb[oPB + r] = v;
                            continue;
                        }
                        r -= nx * nu;
                        Acc v_acc = tb[op + r];
                        for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(tb[oP + r * nx + k], gc[t * nx + k], v_acc);
                        const T v = (T)v_acc;
                        tb[oPc + r] = v;
                    }
                    wsync();
                    // Quu, qu, Qux
                    for (int e = lane; e < nu * nu + nu + nu * nx; e += 64) {
                        int r = e;
                        if (r < nu * nu) {
                            const int i = r / nu, j = r - i * nu;
                            T ga = T(0), ha = T(0);
                            if (i == j) ha = bh[uo + t * nu + i];
                            Acc v_acc = Rs[i * nu + j] + Wt[(nx + i) * nin + nx + j] + (i == j ? ha + reg : T(0));
                            for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(At[k * nin + nx + i], tb[oPB + k * nu + j], v_acc);
                            const T v = (T)v_acc;
                            tb[oQuu + r] = v;
                            continue;
                        }
                        r -= nu * nu;
                        if (r < nu) {
                            T ga = T(0), ha = T(0);
                            ha = bh[uo + t * nu + r];
                            Acc v_acc = gr[uo + t * nu + r] + ga;
                            for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(At[k * nin + nx + r], tb[oPc + k], v_acc);
                            const T v = (T)v_acc;
                            tb[oqu + r] = v;
                            continue;
                        }
                        r -= nu;
                        if (t > 0) {
                            const int i = r / nx, j = r - i * nx;
                            Acc w_acc = Wt[(nx + i) * nin + j];
                            for (int k = 0; k < nx; ++k) w_acc = lq_fma<Acc>(At[k * nin + nx + i], tb[oPA + k * nx + j], w_acc);
                            const T w = (T)w_acc;
                            tb[oQux + r] = w;
                        }
                    }
                    wsync();
                    // Cholesky Quu = L L' (lower, in place): small and serial, one lane
                    if (lane == 0) {
                        T ok = T(1);
                        for (int j = 0; j < nu && ok > T(0); ++j) {
                            T d = tb[oQuu + j * nu + j];
                            for (int k = 0; k < j; ++k) d -= tb[oQuu + j * nu + k] * tb[oQuu + j * nu + k];
                            if (!(d > T(1e-12))) { ok = T(0); break; }
                            d = inv_sqrt_pos(d);              // inverse diagonal, as in the thread-per-problem kernel
                            tb[oQuu + j * nu + j] = d;
                            for (int i = j + 1; i < nu; ++i) {
                                T v = tb[oQuu + i * nu + j];
                                for (int k = 0; k < j; ++k) v -= tb[oQuu + i * nu + k] * tb[oQuu + j * nu + k];
                                tb[oQuu + i * nu + j] = v * d;
                            }
                        }
                        tb[oflag] = ok;
                    }
                    wsync();
                    if (!(tb[oflag] > T(0))) { pd = false; break; }
                    // kv = -Quu^-1 qu ; K = -Quu^-1 Qux: one right-hand side per lane (lane 0: qu, lane 1+col: Qux[:,col]);
                    // the substitution runs in a per-lane strip of the du scratch (nu entries per column)
                    const int ncolK = t > 0 ? nx : 0;
                    for (int c1 = lane; c1 <= ncolK; c1 += 64) {
                        const int col = c1 - 1;
                        T* y = tb + oflag + 1 + c1 * nu;       // per-column work vector
                        for (int i = 0; i < nu; ++i) {
                            T v = (col < 0) ? tb[oqu + i] : tb[oQux + i * nx + col];
                            for (int k = 0; k < i; ++k) v -= tb[oQuu + i * nu + k] * y[k];
                            y[i] = v * tb[oQuu + i * nu + i];
                        }
                        for (int i = nu - 1; i >= 0; --i) {
                            T v = y[i];
                            for (int k = i + 1; k < nu; ++k) v -= tb[oQuu + k * nu + i] * y[k];
                            v *= tb[oQuu + i * nu + i];
                            y[i] = v;
                        }
                        for (int i = 0; i < nu; ++i) {
                            if (col < 0) { tb[okv + i] = -y[i]; kst[(size_t)t * nu + i] = -y[i]; }
                            else { tb[oK + i * nx + col] = -y[i]; Kst[(size_t)t * nu * nx + i * nx + col] = -y[i]; }
                        }
                    }
                    wsync();
                    if (t > 0) {
                        for (int e = lane; e < nx * nx + nx; e += 64) {
                            if (e < nx * nx) {
                                const int i = e / nx, j = e - i * nx;
                                T ga = T(0), ha = T(0);
                                if (i == j) ha = bh[(t - 1) * nx + i];
                                Acc v_acc = Qs[i * nx + j] + Wt[i * nin + j] + (i == j ? ha : T(0));
                                for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(At[k * nin + i], tb[oPA + k * nx + j], v_acc);
                                for (int k = 0; k < nu; ++k) v_acc = lq_fma<Acc>(tb[oQux + k * nx + i], tb[oK + k * nx + j], v_acc);
                                const T v = (T)v_acc;
                                tb[oPn + e] = v;
                            } else {
                                const int i = e - nx * nx;
                                T ga = T(0), ha = T(0);
                                ha = bh[(t - 1) * nx + i];
                                Acc v_acc = gr[(t - 1) * nx + i] + ga;
                                for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(At[k * nin + i], tb[oPc + k], v_acc);
                                for (int k = 0; k < nu; ++k) v_acc = lq_fma<Acc>(tb[oQux + k * nx + i], tb[okv + k], v_acc);
                                const T v = (T)v_acc;
                                tb[opn + i] = v;
                            }
                        }
                        wsync();
                        for (int e = lane; e < nx * nx + nx; e += 64) {
                            if (e < nx * nx) {
                                const int i = e / nx, j = e - i * nx;
                                tb[oP + e] = T(0.5) * (tb[oPn + i * nx + j] + tb[oPn + j * nx + i]);
                            } else {
                                tb[op + e - nx * nx] = tb[opn + e - nx * nx];
                            }
                        }
                        wsync();
                    }
                }
                if (pd) { solved = true; break; }
                reg = fmax(reg * (T)a.reg_raise, T(NEMPC_REG_FLOOR));     // as in the thread-per-problem kernel
                ++restarts;
            }
            if (lane == 0) ((T*)a.reg)[b] = reg;
            if (!solved) {
                // out of attempts: no step this iteration (see the thread-per-problem kernel)
                for (int i = lane; i < n; i += 64) dz[i] = T(0);
                const T* lcur = (const T*)a.lam + (size_t)b * a.m;
                for (int i = lane; i < H * nx; i += 64) lamn[i] = lcur[i];
                if (lane == 0) {
                    T* info = (T*)a.info + (size_t)b * INFO_N;
                    info[INFO_STEP] = std::numeric_limits<T>::max();
                    info[INFO_RESTARTS] = (T)(-restarts);
                }
            } else {
            // forward sweep; the norms are accumulated per lane and reduced at the end
            T lam_inf = T(0), step_inf = T(0), amax = T(1), D0 = T(0), g1 = T(0), ginf = T(0), zinf = T(0);
            const T tau = T(0.995);
            for (int i = lane; i < nx; i += 64) tb[odx + i] = T(0);
            wsync();
            for (int t = 0; t < H; ++t) {
                const T* At = tl + (size_t)t * nx * nin;
                for (int i = lane; i < nu; i += 64) {
                    Acc v_acc = kst[(size_t)t * nu + i];
                    if (t > 0)
                        for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(Kst[(size_t)t * nu * nx + i * nx + k], tb[odx + k], v_acc);
                    const T v = (T)v_acc;
                    tb[odu + i] = v;
                }
                wsync();
                for (int i = lane; i < nx; i += 64) {
                    Acc v_acc = gc[t * nx + i];
                    if (t > 0)
                        for (int k = 0; k < nx; ++k) v_acc = lq_fma<Acc>(At[i * nin + k], tb[odx + k], v_acc);
                    for (int k = 0; k < nu; ++k) v_acc = lq_fma<Acc>(At[i * nin + nx + k], tb[odu + k], v_acc);
                    const T v = (T)v_acc;
                    tb[odxn + i] = v;
                }
                wsync();
                for (int i = lane; i < nx + nu; i += 64) {
                    if (i < nx) {
                        Acc lam_acc = pst[(size_t)t * nx + i];
                        for (int k = 0; k < nx; ++k) lam_acc = lq_fma<Acc>(Pst[(size_t)t * nx * nx + i * nx + k], tb[odxn + k], lam_acc);
                        const T lam = (T)lam_acc;
                        lam_inf = fmax(lam_inf, fabs(lam));
                        lamn[t * nx + i] = lam;
                        const T d = tb[odxn + i], zz = z[t * nx + i], lo = lb[t * nx + i], hi = ub[t * nx + i];
                        dz[t * nx + i] = d;
                        step_inf = fmax(step_inf, fabs(d));
                        zinf = fmax(zinf, fabs(zz));
                        T ga = T(0), ha = T(0);
                                    D0 = fma(gr[t * nx + i] + ga, d, D0);
                        if (d < T(0) && lo > -std::numeric_limits<T>::max()) amax = fmin(amax, tau * (zz - lo) / (-d));
                        if (d > T(0) && hi < std::numeric_limits<T>::max()) amax = fmin(amax, tau * (hi - zz) / d);
                        const T gv = fabs(gc[t * nx + i]);
                        g1 += gv;
                        ginf = fmax(ginf, gv);
                    } else {
                        const int j = i - nx;
                        const T d = tb[odu + j], zz = z[uo + t * nu + j], lo = lb[uo + t * nu + j], hi = ub[uo + t * nu + j];
                        dz[uo + t * nu + j] = d;
                        step_inf = fmax(step_inf, fabs(d));
                        zinf = fmax(zinf, fabs(zz));
                        T ga = T(0), ha = T(0);
                                    D0 = fma(gr[uo + t * nu + j] + ga, d, D0);
                        if (d < T(0) && lo > -std::numeric_limits<T>::max()) amax = fmin(amax, tau * (zz - lo) / (-d));
                        if (d > T(0) && hi < std::numeric_limits<T>::max()) amax = fmin(amax, tau * (hi - zz) / d);
                    }
                }
                wsync();
                for (int i = lane; i < nx; i += 64) tb[odx + i] = tb[odxn + i];
                wsync();
            }
            for (int o = 32; o > 0; o >>= 1) {
                lam_inf = fmax(lam_inf, __shfl_down(lam_inf, o, 64));
                step_inf = fmax(step_inf, __shfl_down(step_inf, o, 64));
                amax = fmin(amax, __shfl_down(amax, o, 64));
                D0 += __shfl_down(D0, o, 64);
                g1 += __shfl_down(g1, o, 64);
                ginf = fmax(ginf, __shfl_down(ginf, o, 64));
                zinf = fmax(zinf, __shfl_down(zinf, o, 64));
            }
            if (lane == 0) {
                T* info = (T*)a.info + (size_t)b * INFO_N;
                info[INFO_LAM] = lam_inf; info[INFO_STEP] = step_inf; info[INFO_AMAX] = amax; info[INFO_G1] = g1;
                info[INFO_GINF] = ginf; info[INFO_D0] = D0; info[INFO_ZINF] = zinf; info[INFO_RESTARTS] = (T)restarts;
            }
            }   // solved
        }
    }
    __syncthreads();
    auto stage_out = [&](T* __restrict__ dst, int per, int dst_stride, int loff) {
        const int tot = np * per;
        T* base = dst + (size_t)b0 * dst_stride;
        for (int i = tid; i < tot; i += 256) {
            const int pp = i / per, e = i - pp * per;
            base[(size_t)pp * dst_stride + e] = lds[(size_t)pp * a.lds_stride + loff + e];
        }
    };
    stage_out((T*)a.dz, n, n, Ldz);
    stage_out((T*)a.lamn, H * nx, a.m, Llam);
}

}  // namespace

}  // namespace nempc
