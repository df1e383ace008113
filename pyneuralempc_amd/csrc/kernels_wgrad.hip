// nempc_weight_grad: gtheta = d/dtheta sum_b keep_b sum_t ( w_{b,t} . Phi_t + lam_{b,t} . (T_t v_{b,[t]}) ), theta = all weights
// and biases (include/nempc.h).  No reference counterpart: the reference never differentiates through its network's weights.
//
// S is the epsilon coefficient of (lam + eps w) . Phi(xi + eps v_[t]; theta), eps^2 = 0, so gtheta is the epsilon part of an
// ordinary reverse-mode weight gradient carried out in dual numbers.  Three launches per chunk of rows (wgrad_plan.h):
//   1. wgrad_rows_kernel   one thread per row: dual forward and dual backward through the network (through the four
//                          weight-shared stages under RK4), leaving per layer and factor row the layer input (a, a.) and the
//                          pre-activation cotangent (d, d.):  dW_l = sum_r a_r (x) d._r + a._r (x) d_r,  db_l = sum_r d._r
//   2. wgrad_gemm_kernel   G_l = A_l' Ddot_l + Adot_l' D_l on the matrix cores, K = the factor rows split over workgroups,
//                          every slice's partial block into its own slab with plain stores
//   3. wgrad_reduce_kernel gtheta = (earlier chunks) + the slabs in slice order
// plus, when `skip` is given, one scan launch per call that numbers the kept problems consecutively (a skipped problem takes
// no factor row at all: nothing of it is read, and the sums are those of the batch without it).  No atomics, no signalling
// between workgroups: the launches are ordered by the stream.
#include "activations.h"
#include "nempc_internal.h"
#include "wgrad_plan.h"

namespace nempc {

namespace {

struct WgNet {
    int nl, nin, nx, ne, kind, nstage;
    int din[NEMPC_MAX_LAYERS], dout[NEMPC_MAX_LAYERS], act[NEMPC_MAX_LAYERS];
    double actp[NEMPC_MAX_LAYERS];
    const void* W[NEMPC_MAX_LAYERS];
    const void* Wt[NEMPC_MAX_LAYERS];
    const void* b[NEMPC_MAX_LAYERS];
    long long offA[NEMPC_MAX_LAYERS], offAd[NEMPC_MAX_LAYERS], offD[NEMPC_MAX_LAYERS], offDd[NEMPC_MAX_LAYERS];
    const void* extra;
    RowGather gk;
};

// kept problems in order: src[0 .. nkept) = their indices, src[B] = nkept.  One workgroup; thread i owns a contiguous run.
__global__ __launch_bounds__(256) void wgrad_scan_kernel(const int32_t* __restrict__ skip, int B, int32_t* __restrict__ src) {
    __shared__ int cnt[256];
    const int tid = threadIdx.x, per = (B + 255) / 256;
    const int b0 = tid * per < B ? tid * per : B, b1 = b0 + per < B ? b0 + per : B;
    int c = 0;
    for (int b = b0; b < b1; ++b) c += skip[b] == 0;
    cnt[tid] = c;
    __syncthreads();
    int at = 0;
    for (int i = 0; i < tid; ++i) at += cnt[i];
    for (int b = b0; b < b1; ++b)
        if (skip[b] == 0) src[at++] = b;
    if (tid == 255) src[B] = at;
}

// One thread per row of the chunk.  crow0: the chunk's first (compacted) row; crows: its rows; fac: the factor region (pitch
// factor rows per feature); scr: (4 maxdim + 4 nx) slots of crows_cap each.
template <typename T>
__global__ __launch_bounds__(64) void wgrad_rows_kernel(WgNet net, T DT, int B, int H, long long crow0, int crows, long long pitch,
                                                         int maxdim, long long scr_pitch, const int32_t* __restrict__ src,
                                                         const T* __restrict__ Z, const T* __restrict__ X0, const T* __restrict__ lam,
                                                         const T* __restrict__ v, const T* __restrict__ w, int m,
                                                         T* __restrict__ fac, T* __restrict__ scr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= crows) return;
    const int nl = net.nl, nx = net.nx, nin = net.nin, ns = net.nstage;
    const long long cr = crow0 + i;
    const int cb = (int)(cr / H), t = (int)(cr % H);
    const int nkept = src ? src[B] : B;
    const size_t f0 = (size_t)i * ns;                        // this row's first factor row
    if (cb >= nkept) {                                       // behind the kept problems: rows of exact zeros
        for (int l = 0; l < nl; ++l)
            for (int s = 0; s < ns; ++s) {
                for (int k = 0; k <= net.din[l]; ++k) {
                    fac[net.offA[l] + (size_t)k * pitch + f0 + s] = T(0);
                    fac[net.offAd[l] + (size_t)k * pitch + f0 + s] = T(0);
                }
                for (int k = 0; k < net.dout[l]; ++k) {
                    fac[net.offD[l] + (size_t)k * pitch + f0 + s] = T(0);
                    fac[net.offDd[l] + (size_t)k * pitch + f0 + s] = T(0);
                }
            }
        return;
    }
    const int b = src ? src[cb] : cb;
    const int n = net.gk.n;
    const T* z = Z + (size_t)b * n;
    const T* wrow = w + ((size_t)b * H + t) * nx;
    const T* lrow = lam ? lam + (size_t)b * m + (size_t)t * nx : nullptr;
    const T* vrow = v ? v + (size_t)b * n : nullptr;
    // scratch: cot[2][2][maxdim] (ping-pong, value | tangent), kout[2][nx] the stage's output, kbar[2][nx] its cotangent
    const size_t R = (size_t)scr_pitch;
    T* cot = scr + i;
    T* kout = scr + (size_t)4 * maxdim * R + i;
    T* kbar = kout + (size_t)2 * nx * R;
    auto COT = [&](int buf, int part, int k) -> T& { return cot[(size_t)((buf * 2 + part) * maxdim + k) * R]; };

    // ---- forward, stage by stage
    for (int s = 0; s < ns; ++s) {
        const size_t fr = f0 + s;
        const T c = s == 0 ? T(0) : (s == 3 ? DT : T(0.5) * DT);
        {   // the network input (xi, xi.) into A_0 / Adot_0
            T* A = fac + net.offA[0] + fr;
            T* Ad = fac + net.offAd[0] + fr;
            for (int d = 0; d < nin; ++d) {
                T x = gather_input<T>(net.gk, z, X0, b, t, d), xd = T(0);
                if (vrow) xd = d < nx ? (t == 0 ? T(0) : vrow[(t - 1) * nx + d]) : vrow[H * nx + t * (nin - nx) + (d - nx)];
                if (s > 0 && d < nx) {
                    x += c * kout[(size_t)d * R];
                    xd += c * kout[(size_t)(nx + d) * R];
                }
                A[(size_t)d * pitch] = x;
                Ad[(size_t)d * pitch] = xd;
            }
            for (int j = 0; j < net.ne; ++j) {
                A[(size_t)(nin + j) * pitch] = ((const T*)net.extra)[((size_t)b * H + t) * net.ne + j];
                Ad[(size_t)(nin + j) * pitch] = T(0);
            }
        }
        for (int l = 0; l < nl; ++l) {
            const T* W = (const T*)net.W[l];
            const T* bias = (const T*)net.b[l];
            const int win = net.din[l], wout = net.dout[l];
            const T* A = fac + net.offA[l] + fr;
            const T* Ad = fac + net.offAd[l] + fr;
            fac[net.offA[l] + (size_t)win * pitch + fr] = T(1);       // the bias column
            fac[net.offAd[l] + (size_t)win * pitch + fr] = T(0);
            const bool last = l == nl - 1;
            T* On = last ? kout : fac + net.offA[l + 1] + fr;          // the layer's output: the next layer's input
            T* Ond = last ? kout + (size_t)nx * R : fac + net.offAd[l + 1] + fr;
            const size_t op = last ? R : (size_t)pitch;
            T* D = fac + net.offD[l] + fr;
            T* Dd = fac + net.offDd[l] + fr;
            for (int jb = 0; jb < wout; jb += 8) {
                T acc[8], accd[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    acc[q] = (jb + q < wout) ? bias[jb + q] : T(0);
                    accd[q] = T(0);
                }
#pragma unroll 4          // (four inputs' loads in flight: the loop is latency-bound at one or two waves per SIMD)
                for (int k = 0; k < win; ++k) {
                    const T a = A[(size_t)k * pitch], ad = Ad[(size_t)k * pitch];
                    const T* wr = W + (size_t)k * wout + jb;
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (jb + q < wout) {
                            acc[q] = fma(a, wr[q], acc[q]);
                            accd[q] = fma(ad, wr[q], accd[q]);
                        }
                }
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (jb + q < wout) {
                        T a, d1, d2;
                        if (act_zbased(net.act[l])) {
                            act_from_z<T>(net.act[l], acc[q], a, d1, d2);
                        } else {
                            a = act_f<T>(net.act[l], acc[q], (T)net.actp[l]);
                            d1 = act_d1<T>(net.act[l], a, (T)net.actp[l]);
                            d2 = act_r2<T>(net.act[l], a, (T)net.actp[l]) * d1;
                        }
                        On[(size_t)(jb + q) * op] = a;
                        Ond[(size_t)(jb + q) * op] = d1 * accd[q];
                        D[(size_t)(jb + q) * pitch] = d1;                 // until the backward pass: s'(z) and s''(z) z.
                        Dd[(size_t)(jb + q) * pitch] = d2 * accd[q];
                    }
            }
        }
    }

    // ---- backward, last stage first.  Cotangent of Phi: (lam, w); of the stage outputs k_s: DT/6 (1, 2, 2, 1) times it, plus
    // c_{s+1} times the state part of the next stage's input cotangent
    const T s6 = DT / T(6);
    for (int s = ns - 1; s >= 0; --s) {
        const size_t fr = f0 + s;
        int cur = 0;
        for (int k = 0; k < nx; ++k) {
            const T l0 = lrow ? lrow[k] : T(0), w0 = wrow[k];
            if (ns == 1) {
                COT(0, 0, k) = l0;
                COT(0, 1, k) = w0;
            } else {
                const T wt = (s == 0 || s == 3) ? s6 : T(2) * s6;
                COT(0, 0, k) = wt * l0 + (s == 3 ? T(0) : kbar[(size_t)k * R]);
                COT(0, 1, k) = wt * w0 + (s == 3 ? T(0) : kbar[(size_t)(nx + k) * R]);
            }
        }
        for (int l = nl - 1; l >= 0; --l) {
            const int win = net.din[l], wout = net.dout[l];
            T* D = fac + net.offD[l] + fr;
            T* Dd = fac + net.offDd[l] + fr;
            for (int j = 0; j < wout; ++j) {
                const T s1 = D[(size_t)j * pitch], q = Dd[(size_t)j * pitch];
                const T ab = COT(cur, 0, j), abd = COT(cur, 1, j);
                D[(size_t)j * pitch] = ab * s1;
                Dd[(size_t)j * pitch] = fma(abd, s1, ab * q);
            }
            // the input's cotangent: every input of a hidden layer; of the first layer the states, and only when an earlier
            // stage reads them
            const int need = l > 0 ? win : (s > 0 ? nx : 0);
            if (!need) continue;
            const T* Wt = (const T*)net.Wt[l];      // (out, in) row-major
            for (int ib = 0; ib < need; ib += 8) {
                T acc[8], accd[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[q] = accd[q] = T(0);
#pragma unroll 4
                for (int j = 0; j < wout; ++j) {
                    const T d = D[(size_t)j * pitch], dd = Dd[(size_t)j * pitch];
                    const T* wr = Wt + (size_t)j * win + ib;
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (ib + q < need) {
                            acc[q] = fma(d, wr[q], acc[q]);
                            accd[q] = fma(dd, wr[q], accd[q]);
                        }
                }
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (ib + q < need) {
                        COT(cur ^ 1, 0, ib + q) = acc[q];
                        COT(cur ^ 1, 1, ib + q) = accd[q];
                    }
            }
            cur ^= 1;
        }
        if (s > 0) {
            const T c = s == 3 ? DT : T(0.5) * DT;
            for (int k = 0; k < nx; ++k) {
                kbar[(size_t)k * R] = c * COT(cur, 0, k);
                kbar[(size_t)(nx + k) * R] = c * COT(cur, 1, k);
            }
        }
    }
}

// the 16 x 16 x 4 matrix instruction of each dtype; lane (i = l & 15, q = l >> 4) holds A[i][k = q] and B[k = q][j = i], and
// register r of the result is C[row(q, r)][l & 15] (the two dtypes differ in row())
template <typename T>
struct WgMma;
template <>
struct WgMma<double> {
    typedef double V4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ V4 mma(double a, double b, V4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int q, int r) { return q + 4 * r; }
};
template <>
struct WgMma<float> {
    typedef float V4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ V4 mma(float a, float b, V4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int q, int r) { return 4 * q + r; }
};

struct WgGemm {
    int nl, npairs;                       // npairs = 1: A' Ddot only (no second-order term)
    long long pitch;
    int kvalid;                           // factor rows of this chunk that the sweep wrote
    int first[NEMPC_MAX_LAYERS + 1];      // wgrad_grid
    int nfeat[NEMPC_MAX_LAYERS], nout[NEMPC_MAX_LAYERS], nbi[NEMPC_MAX_LAYERS], nbj[NEMPC_MAX_LAYERS], ks[NEMPC_MAX_LAYERS];
    int nslices[NEMPC_MAX_LAYERS];        // of this chunk
    long long offA[NEMPC_MAX_LAYERS], offAd[NEMPC_MAX_LAYERS], offD[NEMPC_MAX_LAYERS], offDd[NEMPC_MAX_LAYERS];
    long long slab_off[NEMPC_MAX_LAYERS], theta_off[NEMPC_MAX_LAYERS];
};

// One workgroup = one WG_BLOCK x WG_BLOCK block of G_l over one K slice; wave (wm, wn) owns the 32 x 32 quarter, four 16 x 16
// accumulators.  Operands straight from the factor matrices: lane (i = l & 15, q = l >> 4) loads the V = 16 bytes of
// consecutive factor rows k0 + q V .. + V - 1 of its feature (a feature's four lane groups read one 64-byte run) and feeds
// element e to the e-th MFMA of the step -- A and B agree on which factor row sits in which k slot, and a sum does not care.
// Features beyond the matrix and factor rows beyond kvalid are zeros by select; the loads themselves stay inside the
// pitch (a multiple of every ks), so nothing is read past a row.
template <typename T>
__global__ __launch_bounds__(256) void wgrad_gemm_kernel(WgGemm g, const T* __restrict__ fac, T* __restrict__ slab) {
    constexpr int V = 16 / sizeof(T);
    typedef T Vec __attribute__((ext_vector_type(V)));
    typedef typename WgMma<T>::V4 V4;
    int l = 0;
    while (l + 1 < g.nl && (int)blockIdx.x >= g.first[l + 1]) ++l;
    const int rel = (int)blockIdx.x - g.first[l];
    const int bj = rel % g.nbj[l], bi = (rel / g.nbj[l]) % g.nbi[l], sl = rel / (g.nbj[l] * g.nbi[l]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lq = lane >> 4;
    const int i0 = bi * WG_BLOCK + (wave >> 1) * 32, j0 = bj * WG_BLOCK + (wave & 1) * 32;
    const int nfeat = g.nfeat[l], nout = g.nout[l];
    const int k0 = sl * g.ks[l], k1 = min(k0 + g.ks[l], g.kvalid);
    if (i0 >= nfeat || j0 >= nout) return;       // a quarter outside the matrix (narrow layers): nothing to add, nothing to write
    V4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[a][c] = V4{T(0), T(0), T(0), T(0)};
    const bool ia[2] = {i0 + li < nfeat, i0 + 16 + li < nfeat}, ja[2] = {j0 + li < nout, j0 + 16 + li < nout};
    for (int pr = 0; pr < g.npairs; ++pr) {
        const T* Am = fac + (pr == 0 ? g.offA[l] : g.offAd[l]);
        const T* Bm = fac + (pr == 0 ? g.offDd[l] : g.offD[l]);
        const T* ap[2] = {Am + (size_t)(i0 + li) * g.pitch, Am + (size_t)(i0 + 16 + li) * g.pitch};
        const T* bp[2] = {Bm + (size_t)(j0 + li) * g.pitch, Bm + (size_t)(j0 + 16 + li) * g.pitch};
        // four k steps per trip, their eight loads per lane issued together: a slice is a handful of trips, and one load
        // round trip per step was most of the kernel's time at the headline shape (ks is a multiple of 16 V, so a trip never
        // leaves the slice's ks factor rows, which the pitch holds)
        for (int k = k0; k < k1; k += 16 * V) {
            Vec av[4][2], bv[4][2];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kk = k + u * 4 * V + lq * V;
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    av[u][a] = ia[a] ? *(const Vec*)(ap[a] + kk) : Vec(T(0));
                    bv[u][a] = ja[a] ? *(const Vec*)(bp[a] + kk) : Vec(T(0));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kk = k + u * 4 * V + lq * V;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const bool in = kk + e < k1;
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int c = 0; c < 2; ++c)
                            acc[a][c] = WgMma<T>::mma(in ? av[u][a][e] : T(0), in ? bv[u][c][e] : T(0), acc[a][c]);
                }
            }
        }
    }
    T* out = slab + g.slab_off[l] + (size_t)sl * nfeat * nout;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int fi = i0 + a * 16 + WgMma<T>::row(lq, r), fj = j0 + c * 16 + li;
                if (fi < nfeat && fj < nout) out[(size_t)fi * nout + fj] = acc[a][c][r];
            }
}

// gtheta[e] = (first chunk ? 0 : gtheta[e]) + slab_0[e] + slab_1[e] + ...   in slice order
template <typename T>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(WgGemm g, long long P, int first_chunk, const T* __restrict__ slab,
                                                           T* __restrict__ gtheta) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P) return;
    int l = 0;
    while (l + 1 < g.nl && e >= g.theta_off[l + 1]) ++l;
    const long long sz = (long long)g.nfeat[l] * g.nout[l];
    const T* sp = slab + g.slab_off[l] + (e - g.theta_off[l]);
    T acc = first_chunk ? T(0) : gtheta[e];
    const int ns = g.nslices[l];
    int s = 0;
    for (; s + 8 <= ns; s += 8) {          // eight loads in flight, added in slice order all the same
        T x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = sp[(size_t)(s + q) * sz];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc += x[q];
    }
    for (; s < ns; ++s) acc += sp[(size_t)s * sz];
    gtheta[e] = acc;
}

WgradShape shape_of(const Handle& h) {
    WgradShape s{};
    s.nl = h.nl; s.nstage = h.cfg.integrator == NEMPC_RK4 ? 4 : 1; s.num_cus = h.num_cus; s.esz = h.esz;
    for (int l = 0; l < h.nl; ++l) { s.din[l] = h.din[l]; s.dout[l] = h.dout[l]; }
    return s;
}

size_t align256(size_t x) { return (x + 255) / 256 * 256; }

template <typename T>
int run(Handle& h, const WgradPlan& p, int B, const void* Z, const void* X0, const void* lam, const void* v, const void* w,
        const int32_t* skip, void* gtheta, hipStream_t s) {
    const int H = h.cfg.H, nx = h.cfg.nx;
    const size_t scr_elems = (size_t)(4 * p.maxdim + 4 * nx) * p.chunk_rows;
    char* base = h.d_wgrad_ws.as<char>();
    T* fac = (T*)base;
    T* scr = (T*)(base + align256((size_t)p.factor_elems * sizeof(T)));
    T* slab = (T*)((char*)scr + align256(scr_elems * sizeof(T)));
    int32_t* src = (int32_t*)((char*)slab + align256((size_t)p.slab_elems * sizeof(T)));
    if (skip) {
        hipLaunchKernelGGL(wgrad_scan_kernel, dim3(1), dim3(256), 0, s, skip, B, src);
        NEMPC_HIP(hipGetLastError());
    }
    WgNet net{};
    net.nl = h.nl; net.nin = h.nin; net.nx = nx; net.ne = h.ne; net.kind = h.cfg.integrator; net.nstage = p.nstage;
    net.extra = h.d_extra; net.gk = h.gather();
    WgGemm g{};
    g.nl = h.nl; g.npairs = v ? 2 : 1; g.pitch = p.pitch;
    for (int l = 0; l < h.nl; ++l) {
        net.din[l] = h.din[l]; net.dout[l] = h.dout[l]; net.act[l] = h.act[l]; net.actp[l] = h.actp[l];
        net.W[l] = h.d_W[l].get(); net.Wt[l] = h.d_Wt[l].get(); net.b[l] = h.d_b[l].get();
        const WgradLayer& L = p.L[l];
        net.offA[l] = g.offA[l] = L.offA; net.offAd[l] = g.offAd[l] = L.offAd;
        net.offD[l] = g.offD[l] = L.offD; net.offDd[l] = g.offDd[l] = L.offDd;
        g.nfeat[l] = L.nfeat; g.nout[l] = L.nout; g.nbi[l] = L.nbi; g.nbj[l] = L.nbj; g.ks[l] = L.ks;
        g.slab_off[l] = L.slab_off; g.theta_off[l] = L.theta_off;
    }
    const long long rows = (long long)B * H, nchunks = wgrad_num_chunks(p, rows);
    for (long long c = 0; c < nchunks; ++c) {
        long long r0, r1;
        wgrad_chunk(p, rows, c, r0, r1);
        const int crows = (int)(r1 - r0);
        hipLaunchKernelGGL(wgrad_rows_kernel<T>, dim3((crows + 63) / 64), dim3(64), 0, s, net, (T)h.cfg.DT, B, H, r0, crows,
                           p.pitch, p.maxdim, p.chunk_rows, skip ? src : (const int32_t*)nullptr, (const T*)Z, (const T*)X0,
                           (const T*)lam, (const T*)v, (const T*)w, h.m, fac, scr);
        NEMPC_HIP(hipGetLastError());
        long long first[NEMPC_MAX_LAYERS + 1];
        const long long grid = wgrad_grid(p, crows, first);
        g.kvalid = crows * p.nstage;
        for (int l = 0; l <= h.nl; ++l) g.first[l] = (int)first[l];
        for (int l = 0; l < h.nl; ++l) g.nslices[l] = wgrad_slices(p, l, crows);
        hipLaunchKernelGGL(wgrad_gemm_kernel<T>, dim3((unsigned)grid), dim3(256), 0, s, g, (const T*)fac, slab);
        NEMPC_HIP(hipGetLastError());
        hipLaunchKernelGGL(wgrad_reduce_kernel<T>, dim3((unsigned)((p.P + 255) / 256)), dim3(256), 0, s, g, p.P, (int)(c == 0),
                           (const T*)slab, (T*)gtheta);
        NEMPC_HIP(hipGetLastError());
    }
    return NEMPC_OK;
}

}  // namespace

long long wgrad_n_params(const Handle& h) { return wgrad_n_params(shape_of(h)); }

// The checked call (nempc_api.hip).  The workspace -- factors, sweep scratch, slabs, the kept-problem list -- belongs to the
// handle and is allocated, or grown, by the call that needs it: such a call synchronises the device.
int launch_weight_grad(Handle& h, int B, const void* Z, const void* X0, const void* lam, const void* v, const void* w,
                       const int32_t* skip, void* gtheta, hipStream_t s) {
    const long long req = env_int("NEMPC_WGRAD_CHUNK_ROWS", 0);
    const WgradPlan p = wgrad_make_plan(shape_of(h), (long long)h.cfg.max_batch * h.cfg.H, req);
    long long first[NEMPC_MAX_LAYERS + 1];
    if (wgrad_grid(p, p.chunk_rows, first) > 0x7fffffffll || p.pitch > 0x7fffffffll) {
        set_error("nempc_weight_grad: the chunk is too large for one launch (lower NEMPC_WGRAD_CHUNK_ROWS)");
        return NEMPC_EINVAL;
    }
    const size_t bytes = align256((size_t)p.factor_elems * h.esz) + align256((size_t)(4 * p.maxdim + 4 * h.cfg.nx) * p.chunk_rows * h.esz) +
                         align256((size_t)p.slab_elems * h.esz) + align256(((size_t)h.cfg.max_batch + 1) * sizeof(int32_t));
    if (int rc = h.d_wgrad_ws.ensure(bytes, "nempc_weight_grad workspace")) return rc;
    return h.cfg.dtype == NEMPC_F64 ? run<double>(h, p, B, Z, X0, lam, v, w, skip, gtheta, s)
                                    : run<float>(h, p, B, Z, X0, lam, v, w, skip, gtheta, s);
}

}  // namespace nempc
