// Forward simulation (nempc_rollout): x_t = Phi(x_{t-1}, u_t), t = 0 .. H-1, x_{-1} = X0 -- serial in t, parallel in B.
//
// The row kernels evaluate all B*H rows of the multiple-shooting problem at GIVEN states; here step t reads the state step
// t-1 of the same launch produced, so one launch walks the whole horizon and the states never travel through memory between
// steps: they are written to Z on the way (the result) and kept in a per-wave LDS ring of the last w+1 entries of
// [x0 ; x_0 ; x_1 ; ...] (w = rolling window; w = 1: just x_{t-1}), which is all a row's input gather can reach.  The
// states in Z are never read.  Phi is the row kernels' map (kernels_valu.hip): Discret / Unity / RK4 with u and the extra
// inputs held over the four stages, rolling windows in both orders, any activation on any layer.  Forward only: no s', s''
// slots, no reverse sweep, no tiles.
//
// Two kernels:
//   rollout_mfma_kernel  one wave owns 16 problems for all H steps.  The operand arrangement of kernels_mfma_impl.h:
//                        weights are the MFMA A operand (features on M), activations the B operand (problems on N), so the
//                        accumulator of v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 (col = lane & 15 the problem, row
//                        = MfmaOps<T>::row(lane >> 4, reg) the feature) IS the next layer's B operand: k-step (mo, r) of
//                        the next layer takes accumulator register r of block mo as it stands, and the weight element a
//                        lane loads for it is W[16 mo + row(lane >> 4, r)][16 mo' + (lane & 15)].  Activations stay in
//                        registers through the whole network.  The activation of a layer is a run-time code behind a
//                        wave-uniform switch (forward only: nothing downstream needs it at compile time), hence any
//                        per-layer mix, the z-based codes and non-linear output layers.  Weight fragments are formed from
//                        d_W[l] (in, out) row-major -- the 16 lanes of a k row read 16 consecutive elements -- not from the
//                        packed blob (a handle has one only on the NEMPC_KERNEL_MFMA variant, laid out for ONE padded
//                        width and one activation family), and staged in LDS once per workgroup (below).  Hidden widths
//                        <= 128, <= 4 hidden layers, nx <= 16, network inputs <= 32; widths and input counts off the
//                        16 / 4 grid are zero-padded (a padded unit has z = 0, a finite activation, and zero weights
//                        into the next layer).  Up to four waves (tiles) per workgroup once there are more tiles than
//                        compute units.
//   rollout_wave_kernel  any dims: one wave per problem, lanes over the output units of a layer (W[i][j .. j+63]
//                        coalesced), the two activation vectors ping-pong in LDS, the input vector in a third buffer (RK4
//                        re-reads u and the extras in every stage).
#include <algorithm>

#include "activations.h"
#include "kernels_mfma_impl.h"
#ifdef NEMPC_TILE_STRONG_SYNC
#error "kernels_rollout.hip: wave_sync must be wave-local here (waves of a workgroup leave at different points)"
#endif
#include "nempc_internal.h"

namespace nempc {

namespace {

constexpr int kRollMaxIn = 32;       // matrix-core kernel: network inputs (window + extras), two 16-row blocks
constexpr int kRollMaxNx = 16;
constexpr int kRollMaxHidden = 4;
constexpr int kRollMaxWidth = 128;

struct RollNet {
    int nl, nin, ne, nx, nu, H, kind, B;
    double DT;
    RowGather gk;
    const void* extra;               // (B,H,ne) or null
    int din[NEMPC_MAX_LAYERS], dout[NEMPC_MAX_LAYERS], act[NEMPC_MAX_LAYERS];
    double actp[NEMPC_MAX_LAYERS];
    const void* W[NEMPC_MAX_LAYERS];   // (in, out) row-major
    const void* b[NEMPC_MAX_LAYERS];
};

template <typename T>
__device__ __forceinline__ T roll_act(int code, T z, T par) {
    if (act_zbased(code)) {
        T a, d1, d2;
        act_from_z<T>(code, z, a, d1, d2);
        return a;
    }
    return act_f<T>(code, z, par);
}

// gather_input (nempc_internal.h) with the states taken from the ring instead of z: entry tau >= 0 of [x0 ; states],
// component c, lives at ring[((tau % (w+1)) * nx + c) * rs].  z is read for controls only.
template <typename T>
__device__ __forceinline__ T roll_input(const RowGather& gk, const T* __restrict__ z, const T* ring, int rs, int b, int t, int d) {
    const int nx = gk.nx, nu = gk.nu, w1 = gk.w + 1;
    if (gk.w == 1) {
        if (d < nx) return ring[((t % w1) * nx + d) * rs];
        return z[gk.H * nx + t * nu + (d - nx)];
    }
    const int wx = gk.w * nx, back = gk.w - 1;
    if (d < wx) {
        const int j = d / nx, c = d - j * nx;
        const int tau = t + (gk.rev ? -j : j - back);
        if (tau >= 0) return ring[((tau % w1) * nx + c) * rs];
        return static_cast<const T*>(gk.hx)[((size_t)b * back + (back + tau)) * nx + c];
    }
    d -= wx;
    const int j = d / nu, c = d - j * nu;
    const int tau = t + (gk.rev ? -j : j - back);
    if (tau >= 0) return z[gk.H * nx + tau * nu + c];
    return static_cast<const T*>(gk.hu)[((size_t)b * back + (back + tau)) * nu + c];
}

// ---------------------------------------------------------------------------------------------------------- matrix-core
// Weight fragments.  k-step ks = 4 mt + r of layer l, output block mo: lane (q, c) holds W_l[16 mt + row(q, r)][16 mo + c]
// (0 off the matrix).  WLDS: the workgroup stages every layer's fragments once, lane-linear (element ((ks mo_n + mo) 64 +
// lane) of the layer's region: one conflict-free ds_read per matrix instruction), and the biases zero-padded to 16 behind
// them -- the same weights serve all H steps (x 4 RK4 stages) of every tile of the workgroup.  !WLDS (the fragments do not fit the LDS): the same
// elements by predicated loads from d_W[l] at their point of use.
__host__ __device__ inline int roll_pad16(int v) { return (v + 15) & ~15; }

template <typename T>
__device__ __forceinline__ void roll_stage_weights(const RollNet& net, T* wl, T* bl, int tid, int nthreads) {
    using Ops = MfmaOps<T>;
    const int lane = tid & 63, c = lane & 15, q = lane >> 4, wv = tid >> 6, nw = nthreads >> 6;
    int woff = 0, boff = 0;
    for (int l = 0; l < net.nl; ++l) {
        const int din = net.din[l], dout = net.dout[l];
        const int kt = (din + 15) >> 4, mo_n = (dout + 15) >> 4, nfrag = kt * 4 * mo_n;
        const T* __restrict__ W = static_cast<const T*>(net.W[l]);
        const T* __restrict__ bias = static_cast<const T*>(net.b[l]);
#pragma unroll 4
        for (int fi = wv; fi < nfrag; fi += nw) {
            const int ks = fi / mo_n, mo = fi - ks * mo_n;
            const int k = 16 * (ks >> 2) + Ops::row(q, ks & 3), m = 16 * mo + c;
            wl[woff + fi * 64 + lane] = (k < din && m < dout) ? W[(size_t)k * dout + m] : T(0);
        }
        for (int e = tid; e < mo_n * 16; e += nthreads) bl[boff + e] = e < dout ? bias[e] : T(0);
        woff += nfrag * 64;
        boff += mo_n * 16;
    }
}

// the network at the inputs in s_xi ([d][16 problems]); returns the output layer's accumulator: feature row(q, r), problem c
template <typename T, int MO, bool WLDS>
__device__ __forceinline__ typename MfmaOps<T>::V4 roll_forward_mfma(const RollNet& net, const T* s_xi, T* s_act, const T* wl,
                                                                     const T* bl, int lane) {
    using Ops = MfmaOps<T>;
    using V4 = typename Ops::V4;
    constexpr int MB = MO < 2 ? 2 : MO;
    const int c = lane & 15, q = lane >> 4;
    V4 bop[MB], acc[MO];
#pragma unroll
    for (int mt = 0; mt < MB; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) bop[mt][r] = mt < 2 ? s_xi[(16 * mt + Ops::row(q, r)) * 16 + c] : T(0);
    int woff = 0, boff = 0;
    for (int l = 0; l < net.nl; ++l) {
        const int din = net.din[l], dout = net.dout[l];
        const int kt = (din + 15) >> 4, mo_n = (dout + 15) >> 4;
        const T* __restrict__ W = static_cast<const T*>(net.W[l]);
        const T* __restrict__ bias = static_cast<const T*>(net.b[l]);
#pragma unroll
        for (int mo = 0; mo < MO; ++mo)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * mo + Ops::row(q, r);
                if constexpr (WLDS) acc[mo][r] = mo < mo_n ? bl[boff + f] : T(0);
                else acc[mo][r] = f < dout ? bias[f] : T(0);
            }
#pragma unroll
        for (int mt = 0; mt < MB; ++mt) {
            if (mt >= kt) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (16 * mt + Ops::row(0, r) >= din) continue;      // (wave-uniform: no lane of this k-step has an input)
                const int k = 16 * mt + Ops::row(q, r);
                T wv[MO];
#pragma unroll
                for (int mo = 0; mo < MO; ++mo) {
                    if constexpr (WLDS) {
                        wv[mo] = mo < mo_n ? wl[woff + (((mt * 4 + r) * mo_n + mo) * 64 + lane)] : T(0);
                    } else {
                        const int m = 16 * mo + c;
                        wv[mo] = (k < din && m < dout) ? W[(size_t)k * dout + m] : T(0);
                    }
                }
#pragma unroll
                for (int mo = 0; mo < MO; ++mo)
                    if (mo < mo_n) acc[mo] = Ops::mma(wv[mo], bop[mt][r], acc[mo]);
            }
        }
        const int code = net.act[l];
        const T par = (T)net.actp[l];
        if (code != NEMPC_ACT_LINEAR) {
            // the activation in ONE rolled loop over the lane's own LDS slots: unrolled over the accumulator registers the
            // 14-way switch would be inlined 4 MO times
#pragma unroll
            for (int mo = 0; mo < MO; ++mo)
                if (mo < mo_n) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) s_act[(mo * 4 + r) * 64 + lane] = acc[mo][r];
                }
#pragma unroll 1
            for (int e = 0; e < mo_n * 4; ++e) s_act[e * 64 + lane] = roll_act<T>(code, s_act[e * 64 + lane], par);
#pragma unroll
            for (int mo = 0; mo < MO; ++mo)
                if (mo < mo_n) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[mo][r] = s_act[(mo * 4 + r) * 64 + lane];
                }
        }
#pragma unroll
        for (int mo = 0; mo < MO; ++mo) bop[mo] = acc[mo];
        woff += kt * 4 * mo_n * 64;
        boff += mo_n * 16;
    }
    return acc[0];
}

// dynamic LDS (elements): [WLDS: fragments wtot | biases btot] then per wave: xi[32][16] | ring[(w + 1) nx][16] | act[4 MO][64]
template <typename T, int MO, bool WLDS>
__global__ __launch_bounds__(256) void rollout_mfma_kernel(RollNet net, int wtot, int btot, const T* __restrict__ X0,
                                                           const T* __restrict__ Zc, T* __restrict__ Zs) {
    using Ops = MfmaOps<T>;
    using V4 = typename Ops::V4;
    extern __shared__ __attribute__((aligned(16))) unsigned char roll_mfma_lds_raw[];
    T* wl = reinterpret_cast<T*>(roll_mfma_lds_raw);
    T* bl = wl + (WLDS ? wtot : 0);
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int B = net.B, H = net.H, nx = net.nx, nin = net.nin, k0 = net.nin + net.ne, n = net.gk.n;
    const int w1 = net.gk.w + 1;
    T* s_xi = bl + (WLDS ? btot : 0) + wave * ((kRollMaxIn + w1 * nx) * 16 + 4 * MO * 64);
    T* s_ring = s_xi + kRollMaxIn * 16;
    T* s_act = s_ring + w1 * nx * 16;
    if constexpr (WLDS) {
        roll_stage_weights<T>(net, wl, bl, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const int b0 = (blockIdx.x * nwaves + wave) * 16;        // one wave, one tile of 16 problems, all H steps
    // (a wave without a tile leaves here: everything below synchronises with wave_sync, which must stay wave-local --
    // kernels_mfma_impl.h's NEMPC_TILE_STRONG_SYNC form of it, a workgroup barrier, is not for this kernel)
    if (b0 >= B) return;
    const int b = b0 + c;
    const bool valid = b < B;
    const bool rk4 = net.kind == NEMPC_RK4;
    const T DT = (T)net.DT;

    for (int e = lane; e < 16 * nx; e += 64) {            // ring entry 0 = x0
        const int i = e >> 4, bp = b0 + (e & 15);
        s_ring[e] = bp < B ? X0[(size_t)bp * nx + i] : T(0);
    }
    wave_sync();
    for (int t = 0; t < H; ++t) {
        for (int e = lane; e < kRollMaxIn * 16; e += 64) {
            const int d = e >> 4, cp = e & 15, bp = b0 + cp;
            T v = T(0);
            if (bp < B && d < k0)
                v = d < nin ? roll_input<T>(net.gk, Zc + (size_t)bp * n, s_ring + cp, 16, bp, t, d)
                            : static_cast<const T*>(net.extra)[((size_t)bp * H + t) * net.ne + (d - nin)];
            s_xi[e] = v;
        }
        wave_sync();
        const T* xprev = s_ring + (t % w1) * nx * 16 + c;        // x_{t-1}[i] of this lane's problem at xprev[i * 16]
        const int nstages = rk4 ? 4 : 1;
        T xn[4], acck[4] = {T(0), T(0), T(0), T(0)};
        for (int s = 0; s < nstages; ++s) {
            const V4 k = roll_forward_mfma<T, MO, WLDS>(net, s_xi, s_act, wl, bl, lane);
            if (!rk4) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = Ops::row(q, r);
                    xn[r] = i < nx ? (net.kind == NEMPC_DISCRET ? xprev[i * 16] : T(0)) + k[r] : T(0);
                }
                break;
            }
            const T wgt = (s == 1 || s == 2) ? T(2) : T(1);
            const T cn = (s == 2 ? T(1) : T(0.5)) * DT;       // stage s + 1 reads x + cn k_s
            wave_sync();
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = Ops::row(q, r);
                acck[r] = s == 0 ? k[r] : acck[r] + wgt * k[r];
                if (s < 3 && i < nx) s_xi[i * 16 + c] = xprev[i * 16] + cn * k[r];     // (w = 1: x is input 0 .. nx-1)
            }
            wave_sync();
        }
        if (rk4) {
            const T s6 = DT / T(6);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = Ops::row(q, r);
                xn[r] = i < nx ? xprev[i * 16] + s6 * acck[r] : T(0);
            }
        }
        T* xnext = s_ring + ((t + 1) % w1) * nx * 16 + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = Ops::row(q, r);
            if (i < nx) {
                xnext[i * 16] = xn[r];
                if (valid) Zs[(size_t)b * n + (size_t)t * nx + i] = xn[r];
            }
        }
        wave_sync();
    }
}

// -------------------------------------------------------------------------------------------------------------- generic
// LDS (elements): xi[nin + ne] | bufA[maxw] | bufB[maxw] | fo[nx] | kacc[nx] | ring[(w + 1) nx]
template <typename T>
__device__ __forceinline__ void roll_forward_wave(const RollNet& net, const T* xi, T* bufA, T* bufB, T* fo, int lane) {
    const T* in = xi;
    for (int l = 0; l < net.nl; ++l) {
        const int din = net.din[l], dout = net.dout[l];
        const T* __restrict__ W = static_cast<const T*>(net.W[l]);
        const T* __restrict__ bias = static_cast<const T*>(net.b[l]);
        T* out = l == net.nl - 1 ? fo : ((l & 1) ? bufB : bufA);
        const int code = net.act[l];
        const T par = (T)net.actp[l];
        for (int j = lane; j < dout; j += 64) {
            T acc = bias[j];
#pragma unroll 4
            for (int i = 0; i < din; ++i) acc = fma(in[i], W[(size_t)i * dout + j], acc);
            out[j] = roll_act<T>(code, acc, par);
        }
        wave_sync();
        in = out;
    }
}

template <typename T>
__global__ __launch_bounds__(64) void rollout_wave_kernel(RollNet net, int maxw, const T* __restrict__ X0,
                                                          const T* __restrict__ Zc, T* __restrict__ Zs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char roll_lds_raw[];
    T* xi = reinterpret_cast<T*>(roll_lds_raw);
    const int lane = threadIdx.x & 63;
    const int H = net.H, nx = net.nx, nin = net.nin, ne = net.ne, n = net.gk.n, w1 = net.gk.w + 1;
    T* bufA = xi + nin + ne;
    T* bufB = bufA + maxw;
    T* fo = bufB + maxw;
    T* kacc = fo + nx;
    T* ring = kacc + nx;
    const int b = blockIdx.x;
    const T* __restrict__ z = Zc + (size_t)b * n;
    T* __restrict__ zs = Zs + (size_t)b * n;
    const bool rk4 = net.kind == NEMPC_RK4;
    const T DT = (T)net.DT;

    for (int i = lane; i < nx; i += 64) ring[i] = X0[(size_t)b * nx + i];
    wave_sync();
    for (int t = 0; t < H; ++t) {
        for (int d = lane; d < nin; d += 64) xi[d] = roll_input<T>(net.gk, z, ring, 1, b, t, d);
        for (int j = lane; j < ne; j += 64) xi[nin + j] = static_cast<const T*>(net.extra)[((size_t)b * H + t) * ne + j];
        wave_sync();
        const T* xprev = ring + (t % w1) * nx;
        T* xnext = ring + ((t + 1) % w1) * nx;
        if (!rk4) {
            roll_forward_wave<T>(net, xi, bufA, bufB, fo, lane);
            for (int i = lane; i < nx; i += 64) {
                const T v = (net.kind == NEMPC_DISCRET ? xprev[i] : T(0)) + fo[i];
                xnext[i] = v;
                zs[(size_t)t * nx + i] = v;
            }
        } else {
            for (int s = 0; s < 4; ++s) {
                roll_forward_wave<T>(net, xi, bufA, bufB, fo, lane);
                const T wgt = (s == 1 || s == 2) ? T(2) : T(1);
                const T cn = (s == 2 ? T(1) : T(0.5)) * DT;
                for (int i = lane; i < nx; i += 64) {
                    const T k = fo[i];
                    kacc[i] = s == 0 ? k : kacc[i] + wgt * k;
                    if (s < 3) xi[i] = xprev[i] + cn * k;
                }
                wave_sync();
            }
            const T s6 = DT / T(6);
            for (int i = lane; i < nx; i += 64) {
                const T v = xprev[i] + s6 * kacc[i];
                xnext[i] = v;
                zs[(size_t)t * nx + i] = v;
            }
        }
        wave_sync();
    }
}

RollNet make_rollnet(const Handle& h, int B) {
    RollNet r{};
    r.nl = h.nl; r.nin = h.nin; r.ne = h.ne; r.nx = h.cfg.nx; r.nu = h.cfg.nu; r.H = h.cfg.H; r.kind = h.cfg.integrator; r.B = B;
    r.DT = h.cfg.DT;
    r.gk = h.gather();
    r.extra = h.d_extra;
    for (int l = 0; l < h.nl; ++l) {
        r.din[l] = h.din[l]; r.dout[l] = h.dout[l]; r.act[l] = h.act[l]; r.actp[l] = h.actp[l];
        r.W[l] = h.d_W[l].get(); r.b[l] = h.d_b[l].get();
    }
    return r;
}

// LDS plan of the matrix-core kernel: waves (= tiles) per workgroup, whether the weight fragments are staged, bytes
struct RollMfmaPlan {
    int nw, wtot, btot;
    bool wlds;
    size_t bytes;
};
int roll_mfma_mo(const Handle& h) { return (h.maxw <= 64 || h.nl == 1) ? 4 : 8; }
RollMfmaPlan roll_mfma_plan(const Handle& h, int B) {
    RollMfmaPlan p{};
    for (int l = 0; l < h.nl; ++l) {
        p.wtot += roll_pad16(h.din[l]) * roll_pad16(h.dout[l]);
        p.btot += roll_pad16(h.dout[l]);
    }
    const int ntiles = (B + 15) / 16;
    const size_t per_wave = ((size_t)(kRollMaxIn + (h.w + 1) * h.cfg.nx) * 16 + 4 * (size_t)roll_mfma_mo(h) * 64) * h.esz;
    // one tile per compute unit while there are fewer tiles than units; beyond that up to four waves (one per SIMD) share
    // the staged weights of their workgroup
    p.nw = std::min(4, std::max(1, (ntiles + h.num_cus - 1) / h.num_cus));
    const size_t wbytes = (size_t)(p.wtot + p.btot) * h.esz;
    while (p.nw > 1 && wbytes + p.nw * per_wave > h.lds_limit) --p.nw;
    p.wlds = wbytes + p.nw * per_wave <= h.lds_limit;
    p.bytes = (p.wlds ? wbytes : 0) + p.nw * per_wave;
    return p;
}

template <typename T, int MO>
int launch_mfma_mo(const RollNet& net, const RollMfmaPlan& p, int B, const T* x0, T* z, hipStream_t s) {
    const int ntiles = (B + 15) / 16;
    const dim3 block(64 * p.nw), grid((unsigned)((ntiles + p.nw - 1) / p.nw));
    if (p.wlds) {
        NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(&rollout_mfma_kernel<T, MO, true>), p.bytes));
        hipLaunchKernelGGL((rollout_mfma_kernel<T, MO, true>), grid, block, p.bytes, s, net, p.wtot, p.btot, x0, (const T*)z, z);
    } else {
        hipLaunchKernelGGL((rollout_mfma_kernel<T, MO, false>), grid, block, p.bytes, s, net, p.wtot, p.btot, x0, (const T*)z, z);
    }
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

template <typename T>
int launch_mfma_typed(const Handle& h, const RollNet& net, int B, const void* X0, void* Z, hipStream_t s) {
    const RollMfmaPlan p = roll_mfma_plan(h, B);
    const T* x0 = static_cast<const T*>(X0);
    T* z = static_cast<T*>(Z);
    if (roll_mfma_mo(h) == 4) return launch_mfma_mo<T, 4>(net, p, B, x0, z, s);
    return launch_mfma_mo<T, 8>(net, p, B, x0, z, s);
}

template <typename T>
int launch_wave_typed(const Handle& h, const RollNet& net, int B, const void* X0, void* Z, hipStream_t s) {
    const int maxw = h.nl > 1 ? h.maxw : 1;
    const size_t elems = (size_t)h.nin + h.ne + 2 * (size_t)maxw + 2 * (size_t)h.cfg.nx + (size_t)(h.w + 1) * h.cfg.nx;
    const size_t bytes = elems * sizeof(T);
    if (bytes > h.lds_limit) {
        set_error("nempc_rollout: the generic kernel's per-problem vectors do not fit the device's LDS");
        return NEMPC_EUNSUPPORTED;
    }
    NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(&rollout_wave_kernel<T>), bytes));
    const T* x0 = static_cast<const T*>(X0);
    T* z = static_cast<T*>(Z);
    hipLaunchKernelGGL(rollout_wave_kernel<T>, dim3((unsigned)B), dim3(64), bytes, s, net, maxw, x0, (const T*)z, z);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

}  // namespace

bool rollout_mfma_supported(const Handle& h) {
    if (h.cfg.nx > kRollMaxNx || h.nin + h.ne > kRollMaxIn || h.nl - 1 > kRollMaxHidden) return false;
    for (int l = 0; l < h.nl - 1; ++l)
        if (h.dout[l] > kRollMaxWidth) return false;
    return true;
}

int launch_rollout(Handle& h, int B, const void* X0, void* Z, int which, hipStream_t s) {
    const bool fits = rollout_mfma_supported(h);
    if (which == 2 && !fits) {
        set_error("nempc_rollout: NEMPC_ROLLOUT_KERNEL=2, but the matrix-core kernel takes hidden widths <= 128, <= 4 hidden "
                  "layers, nx <= 16 and w*(nx+nu)+n_extra <= 32");
        return NEMPC_EUNSUPPORTED;
    }
    // by shape: the kernel that measured faster (profiles/r08_rollout.txt).  The matrix-core launch is a chain of H x layers
    // dependent layer evaluations per wave and takes the same time from 1 to 4 tiles per compute unit (754 / 763 us at
    // B = 1024 / 16384, 2 x 64 fp64), while the generic kernel's time grows with B (135 / 1237 us): the matrix-core kernel
    // from 2.5 tiles per compute unit on, for hidden widths <= 64 with the weight fragments staged in LDS.  Wider networks
    // (the 8-block instantiation: 24.9 against 2.7 ms at 3 x 128 fp32, B = 1024; 100 against 9.9 ms at 16384) and
    // fragments that do not fit the LDS stay on the generic kernel.  Forced (NEMPC_ROLLOUT_KERNEL=2) it runs on every shape
    // it takes.
    const int ntiles = (B + 15) / 16;
    const bool mfma = which == 2 || (which == 0 && fits && roll_mfma_mo(h) == 4 && 2 * ntiles >= 5 * h.num_cus && roll_mfma_plan(h, B).wlds);
    const RollNet net = make_rollnet(h, B);
    int rc;
    if (mfma) rc = h.cfg.dtype == NEMPC_F64 ? launch_mfma_typed<double>(h, net, B, X0, Z, s) : launch_mfma_typed<float>(h, net, B, X0, Z, s);
    else rc = h.cfg.dtype == NEMPC_F64 ? launch_wave_typed<double>(h, net, B, X0, Z, s) : launch_wave_typed<float>(h, net, B, X0, Z, s);
    if (rc == NEMPC_OK) h.last_rollout_kernel = mfma ? ROLLOUT_MFMA : ROLLOUT_WAVE;
    return rc;
}

}  // namespace nempc
