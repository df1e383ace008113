// Objective + assembly kernels (HBM-bound streaming work; no matrix cores here).
//
//  objective_kernel      f, grad f of the quadratic/linear family   (objective/jax.py:28-41 stand-in)
//  assemble_dense_kernel tiles -> dense (B,m,n) row-major Jacobian  (integrator/discret.py:38-56,
//                        rk4.py:120-176, optimizer/ipopt.py:88-96): every output element is a constant
//                        (0, -1, +1) or one tile element; a per-handle int32 map built once on the host
//                        says which, so the kernel is a pure gather + 16-byte coalesced store stream.
//  assemble_sparse_kernel same map restricted to the structural non-zeros.
//  assemble_hess_*       per-row Lagrangian blocks -> tril values / dense (n,n)  (ipopt.py:66-86)
#include "nempc_internal.h"
#include "kernels_obj_impl.h"
#include "kernels_kkt_impl.h"
#include "bounds_bind_impl.h"
#include "post_plan.h"

namespace nempc {

namespace {

template <typename T>
__device__ __forceinline__ T map_value(int32_t code, const T* __restrict__ tile) {
    if (code >= 0) return tile[code];
    return code == MAP_ZERO ? T(0) : (code == MAP_MINUS_ONE ? T(-1) : T(1));
}

template <typename T>
__global__ __launch_bounds__(64) void objective_kernel(int B, int H, int nx, int nu, ObjOffsets o,
                                                       const T* __restrict__ P, const T* __restrict__ Z,
                                                       T* __restrict__ f, T* __restrict__ grad) {
    if ((int)blockIdx.x < B) objective_body<T>(blockIdx.x, threadIdx.x, H, nx, nu, o, P, Z, f, grad);
}

// objective with per-problem tracking data (nempc_bind_tracking): one wave per row of Z, as objective_kernel; prob (optional)
// maps the row to the caller's problem whose data it is scored against (the solver's compacted batch)
template <typename T>
__global__ __launch_bounds__(64) void objective_tracking_kernel(int B, int H, int nx, int nu, ObjOffsets o,
                                                                const T* __restrict__ P, TrackBind tk,
                                                                const int* __restrict__ prob, const T* __restrict__ Z,
                                                                T* __restrict__ f, T* __restrict__ grad) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const double acc = objective_row_value_tracking<T>(b, prob ? prob[b] : b, lane, H, nx, nu, o, P, tk,
                                                       Z + (size_t)b * (H * (nx + nu)), grad);
    if (f && lane == 0) f[b] = (T)acc;
}

// grid (ceil(m*n / (256 * kAsmVPT * 16/sizeof(T))), B)
// each lane produces VPT x 16 bytes (2 doubles / 4 floats per store), the VPT stores of a lane 256 lanes apart so
// that every store instruction of a wave is contiguous; the map / tile loads of all VPT vectors are issued
// before the first store (memory-level parallelism instead of one dependent L2 round trip per store); kAsmVPT: post_plan.h
template <typename T>
__device__ __forceinline__ void assemble_dense_body(int b, int mn, int tile_elems, const int32_t* __restrict__ map,
                                                    const T* __restrict__ tiles, T* __restrict__ jac) {
    constexpr int NV = 16 / (int)sizeof(T);
    typedef T vecT __attribute__((ext_vector_type(NV)));
    const T* tile = tiles + (size_t)b * tile_elems;
    T* out = jac + (size_t)b * mn;
    const int base = NV * (blockIdx.x * (256 * kAsmVPT) + threadIdx.x);
    int32_t code[kAsmVPT][NV];
#pragma unroll
    for (int u = 0; u < kAsmVPT; ++u) {
        const int e = base + u * 256 * NV;
#pragma unroll
        for (int k = 0; k < NV; ++k) code[u][k] = (e + k < mn) ? map[e + k] : MAP_ZERO;
    }
    T v[kAsmVPT][NV];
#pragma unroll
    for (int u = 0; u < kAsmVPT; ++u)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[u][k] = map_value<T>(code[u][k], tile);
#pragma unroll
    for (int u = 0; u < kAsmVPT; ++u) {
        const int e = base + u * 256 * NV;
        if (e + NV <= mn && (reinterpret_cast<uintptr_t>(out + e) & 15) == 0) {
            vecT vv;
#pragma unroll
            for (int k = 0; k < NV; ++k) vv[k] = v[u][k];
            *reinterpret_cast<vecT*>(out + e) = vv;
        } else {
#pragma unroll
            for (int k = 0; k < NV; ++k)
                if (e + k < mn) out[e + k] = v[u][k];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void assemble_dense_kernel(int mn, int tile_elems, const int32_t* __restrict__ map,
                                                             const T* __restrict__ tiles, T* __restrict__ jac) {
    assemble_dense_body<T>(blockIdx.y, mn, tile_elems, map, tiles, jac);
}

// objective + dense assembly in ONE launch (they are independent; a second launch costs ~1.5 us of
// boundary plus the objective's own ~4.7 us of latency-bound time at B=1024): blocks x < nb_asm stream
// the Jacobian of problem y, the extra block x == nb_asm evaluates the objective of problem y on wave 0.
template <typename T>
__global__ __launch_bounds__(256) void post_kernel(int nb_asm, int mn, int tile_elems, const int32_t* __restrict__ map,
                                                   const T* __restrict__ tiles, T* __restrict__ jac, int H, int nx,
                                                   int nu, ObjOffsets o, const T* __restrict__ P,
                                                   const T* __restrict__ Z, T* __restrict__ f, T* __restrict__ grad) {
    if ((int)blockIdx.x < nb_asm) {
        assemble_dense_body<T>(blockIdx.y, mn, tile_elems, map, tiles, jac);
    } else if (threadIdx.x < 64) {
        objective_body<T>(blockIdx.y, threadIdx.x, H, nx, nu, o, P, Z, f, grad);
    }
}

// Flat variant: the (B, m*n) output is ONE stream of 16-byte vectors cut into full blocks (a per-problem grid leaves
// the last block of every problem mostly idle: m*n = 2400 is 1.17 blocks).  Needs m*n % (16/sizeof(T)) == 0 so that a
// vector never straddles two problems.  Problem index of a vector: one exact division per block, then a
// multiply-high by a host-checked reciprocal for the in-block offset.  Blocks >= nb_asm: objective, one problem per wave.
template <typename T>
__global__ __launch_bounds__(256) void post_flat_kernel(int nb_asm, int B, int mn, unsigned magic, int tile_elems,
                                                        const int32_t* __restrict__ map, const T* __restrict__ tiles,
                                                        T* __restrict__ jac, int H, int nx, int nu, ObjOffsets o,
                                                        const T* __restrict__ P, const T* __restrict__ Z,
                                                        T* __restrict__ f, T* __restrict__ grad) {
    constexpr int NV = 16 / (int)sizeof(T);
    typedef T vecT __attribute__((ext_vector_type(NV)));
    typedef int32_t vecI __attribute__((ext_vector_type(NV)));
    if ((int)blockIdx.x >= nb_asm) {
        const int b = ((int)blockIdx.x - nb_asm) * 4 + (threadIdx.x >> 6);
        if (b < B && (f || grad)) objective_body<T>(b, threadIdx.x & 63, H, nx, nu, o, P, Z, f, grad);
        return;
    }
    const unsigned long long e_blk = (unsigned long long)blockIdx.x * (256 * kAsmVPT * NV);
    const unsigned b_blk = (unsigned)(e_blk / (unsigned)mn);
    const unsigned r_blk = (unsigned)(e_blk - (unsigned long long)b_blk * (unsigned)mn);
    vecI code[kAsmVPT];
    unsigned bb[kAsmVPT], ee[kAsmVPT];
#pragma unroll
    for (int u = 0; u < kAsmVPT; ++u) {
        const unsigned numer = r_blk + (unsigned)(u * 256 + threadIdx.x) * NV;
        const unsigned db = __umulhi(numer, magic);
        ee[u] = numer - db * (unsigned)mn;
        bb[u] = b_blk + db;
        if (bb[u] < (unsigned)B) code[u] = *reinterpret_cast<const vecI*>(map + ee[u]);
    }
    vecT v[kAsmVPT];
#pragma unroll
    for (int u = 0; u < kAsmVPT; ++u) {
        if (bb[u] < (unsigned)B) {
            const T* tile = tiles + (size_t)bb[u] * tile_elems;
#pragma unroll
            for (int k = 0; k < NV; ++k) v[u][k] = map_value<T>(code[u][k], tile);
        }
    }
#pragma unroll
    for (int u = 0; u < kAsmVPT; ++u)
        if (bb[u] < (unsigned)B) *reinterpret_cast<vecT*>(jac + (size_t)bb[u] * mn + ee[u]) = v[u];
}

// host side: can the flat kernel handle (B, mn)?  (post_plan.h: the rule, the reciprocal and why it is exact)
inline bool flat_ok(const Handle& h, int B, const void* jac, unsigned* magic) {
    return post_flat_plan((unsigned)h.m * (unsigned)h.n, B, (unsigned)h.esz, jac, magic) == POST_FLAT_OK;
}

// sparse contract in one launch: band-pattern values for all problems as one flat stream (blocks < nb_asm), objective
// on the blocks after them (one problem per wave).  b = e / nnz by an exact 64-bit multiply-high.
template <typename T>
__global__ __launch_bounds__(256) void post_sparse_kernel(int nb_asm, int B, int nnz, unsigned long long magic64,
                                                          int tile_elems, const int32_t* __restrict__ map,
                                                          const T* __restrict__ tiles, T* __restrict__ vals, int H, int nx,
                                                          int nu, ObjOffsets o, const T* __restrict__ P,
                                                          const T* __restrict__ Z, T* __restrict__ f, T* __restrict__ grad) {
    if ((int)blockIdx.x >= nb_asm) {
        const int b = ((int)blockIdx.x - nb_asm) * 4 + (threadIdx.x >> 6);
        if (b < B) objective_body<T>(b, threadIdx.x & 63, H, nx, nu, o, P, Z, f, grad);
        return;
    }
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (unsigned long long)B * nnz) return;
    const unsigned b = (unsigned)__umul64hi(e, magic64);      // e / nnz, exact for e * nnz < 2^64
    const unsigned k = (unsigned)(e - (unsigned long long)b * nnz);
    vals[e] = map_value<T>(map[k], tiles + (size_t)b * tile_elems);
}

// dense contract into a RESIDENT matrix (nempc_jac_dense_resident: its structural zeros are in place, and so are its constant
// entries -- jac_constants_kernel): the same flat stream over the structural non-zeros, each value that comes from a tile to
// its place in the problem's dense matrix (pos[k] = row * n + col); the objective on the blocks after them when it is asked for.
template <typename T>
__global__ __launch_bounds__(256) void post_scatter_kernel(int nb_asm, int B, int nnz, unsigned long long magic64, int mn,
                                                           int tile_elems, const int32_t* __restrict__ map,
                                                           const int32_t* __restrict__ pos, const T* __restrict__ tiles,
                                                           T* __restrict__ jac, int H, int nx, int nu, ObjOffsets o,
                                                           const T* __restrict__ P, const T* __restrict__ Z,
                                                           T* __restrict__ f, T* __restrict__ grad) {
    if ((int)blockIdx.x >= nb_asm) {
        const int b = ((int)blockIdx.x - nb_asm) * 4 + (threadIdx.x >> 6);
        if (b < B) objective_body<T>(b, threadIdx.x & 63, H, nx, nu, o, P, Z, f, grad);
        return;
    }
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (unsigned long long)B * nnz) return;
    const unsigned b = (unsigned)__umul64hi(e, magic64);      // e / nnz, exact for e * nnz < 2^64
    const unsigned k = (unsigned)(e - (unsigned long long)b * nnz);
    const int32_t code = map[k];
    if (code >= 0) jac[(size_t)b * mn + pos[k]] = tiles[(size_t)b * tile_elems + code];
}

// The constant entries of problems [b0, b0 + count) of a resident dense matrix, written once (jac_resident.h): -1 at (k, k)
// of the hx = H nx defect rows, +1 at (hx + k, k) of the box rows.  One lane per (problem, k).
template <typename T>
__global__ __launch_bounds__(256) void jac_constants_kernel(int b0, int count, int hx, int n, int mn, int box, T* __restrict__ jac) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (unsigned long long)count * hx) return;
    const unsigned b = (unsigned)(e / (unsigned)hx);
    const unsigned k = (unsigned)(e - (unsigned long long)b * hx);
    T* const J = jac + (size_t)(b0 + b) * mn;
    J[(size_t)k * n + k] = T(-1);
    if (box) J[(size_t)(hx + k) * n + k] = T(1);
}

template <typename T>
__global__ __launch_bounds__(256) void assemble_sparse_kernel(int nnz, int tile_elems, const int32_t* __restrict__ map,
                                                              const T* __restrict__ tiles, T* __restrict__ vals) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nnz) vals[(size_t)b * nnz + e] = map_value<T>(map[e], tiles + (size_t)b * tile_elems);
}

// hvals[b][e] = sigma_b * objc[e] + sum_k (map[e][k] >= 0 ? blocks[b][map[e][k]] : 0);  up to w per-row blocks reach
// one entry with a rolling window of w steps (the reference sums them with its projection matrices,
// model/tensorflow.py:312-330); w = 1 for plain models
template <typename T>
__global__ __launch_bounds__(256) void assemble_hess_kernel(int cnt, int w, int blk_elems, const int32_t* __restrict__ map,
                                                            const T* __restrict__ objc, const T* __restrict__ blocks,
                                                            const T* __restrict__ sigma, T* __restrict__ out) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < cnt) {
        T v = sigma[b] * objc[e];
        for (int k = 0; k < w; ++k) {
            const int32_t c = map[(size_t)e * w + k];
            if (c >= 0) v += blocks[(size_t)b * blk_elems + c];
        }
        out[(size_t)b * cnt + e] = v;
    }
}

// The Gauss-Newton form of the same assembly without the intermediate blocks: a block element is formed where it is
// used, from the row kernel's tiles, with gn_blocks_kernel's arithmetic (product first, then the weighted sum over the
// nx outputs of the row) -- one launch and one (B, H, nin, nin) round trip through memory less per callback
template <typename T>
__global__ __launch_bounds__(256) void assemble_hess_gn_kernel(int cnt, int w, int rows, int nx, int nin,
                                                               const int32_t* __restrict__ map, const T* __restrict__ objc,
                                                               const T* __restrict__ tiles, const T* __restrict__ wgt,
                                                               const T* __restrict__ sigma, T* __restrict__ out) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cnt) return;
    const int nn = nin * nin;
    T v = sigma[b] * objc[e];
    for (int k = 0; k < w; ++k) {
        const int32_t c = map[(size_t)e * w + k];
        if (c < 0) continue;
        const int r = c / nn, pq = c - r * nn, p = pq / nin, q = pq - p * nin;
        const T* t = tiles + ((size_t)b * rows + r) * (size_t)(nx * nin);
        const T* wr = wgt ? wgt + ((size_t)b * rows + r) * nx : nullptr;
        T s = T(0);
        for (int i = 0; i < nx; ++i) {
            const T tt = t[i * nin + p] * t[i * nin + q];
            s = fma(wr ? wr[i] : T(1), tt, s);
        }
        v += s;
    }
    out[(size_t)b * cnt + e] = v;
}

}  // namespace

int launch_objective_tracking(Handle& h, int B, const void* Z, void* f, void* grad, const int* prob, hipStream_t s) {
    ObjOffsets o = obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu);
    if (h.cfg.dtype == NEMPC_F64)
        hipLaunchKernelGGL(objective_tracking_kernel<double>, dim3(B), dim3(64), 0, s, B, h.cfg.H, h.cfg.nx, h.cfg.nu, o,
                           h.d_obj.as<const double>(), h.track, prob, (const double*)Z, (double*)f, (double*)grad);
    else
        hipLaunchKernelGGL(objective_tracking_kernel<float>, dim3(B), dim3(64), 0, s, B, h.cfg.H, h.cfg.nx, h.cfg.nu, o,
                           h.d_obj.as<const float>(), h.track, prob, (const float*)Z, (float*)f, (float*)grad);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

int launch_objective(Handle& h, int B, const void* Z, void* f, void* grad, hipStream_t s) {
    if (h.track.on()) return launch_objective_tracking(h, B, Z, f, grad, nullptr, s);
    ObjOffsets o = obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu);
    if (h.cfg.dtype == NEMPC_F64)
        hipLaunchKernelGGL(objective_kernel<double>, dim3(B), dim3(64), 0, s, B, h.cfg.H, h.cfg.nx, h.cfg.nu, o,
                           h.d_obj.as<const double>(), (const double*)Z, (double*)f, (double*)grad);
    else
        hipLaunchKernelGGL(objective_kernel<float>, dim3(B), dim3(64), 0, s, B, h.cfg.H, h.cfg.nx, h.cfg.nu, o,
                           h.d_obj.as<const float>(), (const float*)Z, (float*)f, (float*)grad);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

template <typename T>
int launch_post_flat(Handle& h, int B, unsigned magic, const void* tiles, void* jac, const void* Z, void* f, void* grad,
                     hipStream_t s) {
    const int mn = h.m * h.n;
    const int te = h.cfg.H * h.cfg.nx * h.nin;
    const int nb_asm = post_flat_blocks((unsigned)mn, B, (unsigned)sizeof(T));
    const int nb_obj = (f || grad) ? post_objective_blocks(B) : 0;
    h.last_dense_writer = DENSE_WRITER_FLAT;
    ObjOffsets o = obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu);
    hipLaunchKernelGGL(post_flat_kernel<T>, dim3((unsigned)(nb_asm + nb_obj)), dim3(256), 0, s, nb_asm, B, mn, magic, te,
                       h.d_dense_map.get(), (const T*)tiles, (T*)jac, h.cfg.H, h.cfg.nx, h.cfg.nu, o, h.d_obj.as<const T>(),
                       (const T*)Z, (T*)f, (T*)grad);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

// the structural non-zeros of the dense matrix alone, [+ the objective]: the target is resident (post_scatter_kernel)
template <typename T>
int launch_post_scatter(Handle& h, int B, const void* tiles, void* jac, const void* Z, void* f, void* grad, hipStream_t s) {
    const int nnz = (int)h.jac_rows.size();
    const int te = h.cfg.H * h.cfg.nx * h.nin;
    const int nb_asm = post_nnz_blocks(nnz, B), nb_obj = (f || grad) ? post_objective_blocks(B) : 0;
    unsigned long long magic = 0;
    if (!post_recip64(nnz, &magic)) {
        set_error("launch_post_scatter: a pattern of fewer than two entries");
        return NEMPC_EUNSUPPORTED;
    }
    h.last_dense_writer = DENSE_WRITER_SCATTER;
    ObjOffsets o = obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu);
    hipLaunchKernelGGL(post_scatter_kernel<T>, dim3((unsigned)(nb_asm + nb_obj)), dim3(256), 0, s, nb_asm, B, nnz, magic,
                       h.m * h.n, te, h.d_sparse_map.get(), h.d_sparse_pos.get(), (const T*)tiles, (T*)jac, h.cfg.H, h.cfg.nx, h.cfg.nu, o,
                       h.d_obj.as<const T>(), (const T*)Z, (T*)f, (T*)grad);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

int launch_jac_constants(Handle& h, int b0, int b1, void* jac, hipStream_t s) {
    if (b1 <= b0) return NEMPC_OK;
    const int hx = h.cfg.H * h.cfg.nx, count = b1 - b0;
    const dim3 grid((unsigned)(((size_t)count * hx + 255) / 256)), block(256);
    if (h.cfg.dtype == NEMPC_F64)
        hipLaunchKernelGGL(jac_constants_kernel<double>, grid, block, 0, s, b0, count, hx, h.n, h.m * h.n, h.box ? 1 : 0, (double*)jac);
    else
        hipLaunchKernelGGL(jac_constants_kernel<float>, grid, block, 0, s, b0, count, hx, h.n, h.m * h.n, h.box ? 1 : 0, (float*)jac);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

int launch_assemble_dense(Handle& h, int B, const void* tiles, void* jac, hipStream_t s, bool resident) {
    if (resident)
        return h.cfg.dtype == NEMPC_F64 ? launch_post_scatter<double>(h, B, tiles, jac, nullptr, nullptr, nullptr, s)
                                        : launch_post_scatter<float>(h, B, tiles, jac, nullptr, nullptr, nullptr, s);
    unsigned magic = 0;
    if (flat_ok(h, B, jac, &magic))
        return h.cfg.dtype == NEMPC_F64 ? launch_post_flat<double>(h, B, magic, tiles, jac, nullptr, nullptr, nullptr, s)
                                        : launch_post_flat<float>(h, B, magic, tiles, jac, nullptr, nullptr, nullptr, s);
    const int mn = h.m * h.n;
    const int te = h.cfg.H * h.cfg.nx * h.nin;
    const dim3 block(256), grid((unsigned)post_problem_blocks((unsigned)mn, (unsigned)h.esz), (unsigned)B);
    h.last_dense_writer = DENSE_WRITER_ASSEMBLE;
    if (h.cfg.dtype == NEMPC_F64)
        hipLaunchKernelGGL(assemble_dense_kernel<double>, grid, block, 0, s, mn, te, h.d_dense_map.get(),
                           (const double*)tiles, (double*)jac);
    else
        hipLaunchKernelGGL(assemble_dense_kernel<float>, grid, block, 0, s, mn, te, h.d_dense_map.get(),
                           (const float*)tiles, (float*)jac);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

int launch_post(Handle& h, int B, const void* tiles, void* jac, const void* Z, void* f, void* grad, hipStream_t s,
                bool resident) {
    if (resident)
        return h.cfg.dtype == NEMPC_F64 ? launch_post_scatter<double>(h, B, tiles, jac, Z, f, grad, s)
                                        : launch_post_scatter<float>(h, B, tiles, jac, Z, f, grad, s);
    unsigned magic = 0;
    if (flat_ok(h, B, jac, &magic))
        return h.cfg.dtype == NEMPC_F64 ? launch_post_flat<double>(h, B, magic, tiles, jac, Z, f, grad, s)
                                        : launch_post_flat<float>(h, B, magic, tiles, jac, Z, f, grad, s);
    const int mn = h.m * h.n;
    const int te = h.cfg.H * h.cfg.nx * h.nin;
    const int nb = post_problem_blocks((unsigned)mn, (unsigned)h.esz);
    ObjOffsets o = obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu);
    const dim3 block(256), grid((unsigned)(nb + 1), (unsigned)B);
    h.last_dense_writer = DENSE_WRITER_POST;
    if (h.cfg.dtype == NEMPC_F64)
        hipLaunchKernelGGL(post_kernel<double>, grid, block, 0, s, nb, mn, te, h.d_dense_map.get(), (const double*)tiles,
                           (double*)jac, h.cfg.H, h.cfg.nx, h.cfg.nu, o, h.d_obj.as<const double>(), (const double*)Z,
                           (double*)f, (double*)grad);
    else
        hipLaunchKernelGGL(post_kernel<float>, grid, block, 0, s, nb, mn, te, h.d_dense_map.get(), (const float*)tiles,
                           (float*)jac, h.cfg.H, h.cfg.nx, h.cfg.nu, o, h.d_obj.as<const float>(), (const float*)Z,
                           (float*)f, (float*)grad);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

int launch_post_sparse(Handle& h, int B, const void* tiles, void* vals, const void* Z, void* f, void* grad,
                       hipStream_t s) {
    const int nnz = (int)h.jac_rows.size();
    const int te = h.cfg.H * h.cfg.nx * h.nin;
    const int nb_asm = post_nnz_blocks(nnz, B), nb_obj = post_objective_blocks(B);
    // ceil(2^64 / nnz): floor((2^64 - 1) / nnz) + 1 (post_plan.h; nnz >= 2 always: every row has its -1 and a control column)
    unsigned long long magic = 0;
    if (!post_recip64(nnz, &magic)) {
        set_error("launch_post_sparse: a pattern of fewer than two entries");
        return NEMPC_EUNSUPPORTED;
    }
    ObjOffsets o = obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu);
    if (h.cfg.dtype == NEMPC_F64)
        hipLaunchKernelGGL(post_sparse_kernel<double>, dim3((unsigned)(nb_asm + nb_obj)), dim3(256), 0, s, nb_asm, B, nnz,
                           magic, te, h.d_sparse_map.get(), (const double*)tiles, (double*)vals, h.cfg.H, h.cfg.nx, h.cfg.nu, o,
                           h.d_obj.as<const double>(), (const double*)Z, (double*)f, (double*)grad);
    else
        hipLaunchKernelGGL(post_sparse_kernel<float>, dim3((unsigned)(nb_asm + nb_obj)), dim3(256), 0, s, nb_asm, B, nnz,
                           magic, te, h.d_sparse_map.get(), (const float*)tiles, (float*)vals, h.cfg.H, h.cfg.nx, h.cfg.nu, o,
                           h.d_obj.as<const float>(), (const float*)Z, (float*)f, (float*)grad);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

int launch_assemble_sparse(Handle& h, int B, const void* tiles, void* vals, hipStream_t s) {
    const int nnz = (int)h.jac_rows.size();
    const int te = h.cfg.H * h.cfg.nx * h.nin;
    const dim3 block(256), grid((unsigned)((nnz + 255) / 256), (unsigned)B);
    if (h.cfg.dtype == NEMPC_F64)
        hipLaunchKernelGGL(assemble_sparse_kernel<double>, grid, block, 0, s, nnz, te, h.d_sparse_map.get(),
                           (const double*)tiles, (double*)vals);
    else
        hipLaunchKernelGGL(assemble_sparse_kernel<float>, grid, block, 0, s, nnz, te, h.d_sparse_map.get(),
                           (const float*)tiles, (float*)vals);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

// Gauss-Newton blocks: blocks[r][p][q] = sum_k w[r][k] * T[r][k][p] * T[r][k][q] from the row kernel's tiles T (R, nx, nin);
// w == null means unit weights.  The product T_p * T_q is formed first, so the block is symmetric to the last bit.
template <typename T>
__global__ __launch_bounds__(256) void gn_blocks_kernel(size_t total, int nx, int nin, const T* __restrict__ tiles,
                                                        const T* __restrict__ w, T* __restrict__ blocks) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int nn = nin * nin;
    const size_t r = idx / nn;
    const int pq = (int)(idx - r * nn), p = pq / nin, q = pq - p * nin;
    const T* t = tiles + r * (size_t)(nx * nin);
    T s = T(0);
    for (int k = 0; k < nx; ++k) {
        const T tt = t[k * nin + p] * t[k * nin + q];
        s = fma(w ? w[r * nx + k] : T(1), tt, s);
    }
    blocks[idx] = s;
}

int launch_gn_blocks(Handle& h, int B, const void* tiles, const void* w, void* blocks, hipStream_t s) {
    const size_t total = (size_t)B * h.cfg.H * h.nin * h.nin;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (h.cfg.dtype == NEMPC_F64)
        hipLaunchKernelGGL(gn_blocks_kernel<double>, grid, block, 0, s, total, h.cfg.nx, h.nin, (const double*)tiles,
                           (const double*)w, (double*)blocks);
    else
        hipLaunchKernelGGL(gn_blocks_kernel<float>, grid, block, 0, s, total, h.cfg.nx, h.nin, (const float*)tiles,
                           (const float*)w, (float*)blocks);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

// d_hess_map layout (w codes per entry): [0,nnz) tril map | [nnz, nnz+n*n) dense map ; objc follows the same split in d_hess_objc
int launch_assemble_hess(Handle& h, int B, const void* blocks, const void* sigma, void* hvals, void* hdense,
                         hipStream_t s) {
    const int nnz = (int)h.hess_rows.size();
    const int nn = h.n * h.n;
    const int be = h.cfg.H * h.nin * h.nin;
    const dim3 block(256);
    const size_t esz = h.esz;
    const char* objc = h.d_obj.as<const char>() + (size_t)obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu).total * esz;
    if (hvals) {
        const dim3 grid((unsigned)((nnz + 255) / 256), (unsigned)B);
        if (h.cfg.dtype == NEMPC_F64)
            hipLaunchKernelGGL(assemble_hess_kernel<double>, grid, block, 0, s, nnz, h.w, be, h.d_hess_map.get(),
                               (const double*)objc, (const double*)blocks, (const double*)sigma, (double*)hvals);
        else
            hipLaunchKernelGGL(assemble_hess_kernel<float>, grid, block, 0, s, nnz, h.w, be, h.d_hess_map.get(),
                               (const float*)objc, (const float*)blocks, (const float*)sigma, (float*)hvals);
    }
    if (hdense) {
        const dim3 grid((unsigned)((nn + 255) / 256), (unsigned)B);
        if (h.cfg.dtype == NEMPC_F64)
            hipLaunchKernelGGL(assemble_hess_kernel<double>, grid, block, 0, s, nn, h.w, be, h.d_hess_map.get() + (size_t)nnz * h.w,
                               (const double*)(objc + (size_t)nnz * esz), (const double*)blocks,
                               (const double*)sigma, (double*)hdense);
        else
            hipLaunchKernelGGL(assemble_hess_kernel<float>, grid, block, 0, s, nn, h.w, be, h.d_hess_map.get() + (size_t)nnz * h.w,
                               (const float*)(objc + (size_t)nnz * esz), (const float*)blocks, (const float*)sigma,
                               (float*)hdense);
    }
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

int launch_assemble_hess_gn(Handle& h, int B, const void* tiles, const void* w, const void* sigma, void* hvals, void* hdense,
                            hipStream_t s) {
    const int nnz = (int)h.hess_rows.size();
    const int nn = h.n * h.n;
    const dim3 block(256);
    const size_t esz = h.esz;
    const char* objc = h.d_obj.as<const char>() + (size_t)obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu).total * esz;
    auto go = [&](int cnt, const int32_t* map, const char* oc, void* out) {
        const dim3 grid((unsigned)((cnt + 255) / 256), (unsigned)B);
        if (h.cfg.dtype == NEMPC_F64)
            hipLaunchKernelGGL(assemble_hess_gn_kernel<double>, grid, block, 0, s, cnt, h.w, h.cfg.H, h.cfg.nx, h.nin, map,
                               (const double*)oc, (const double*)tiles, (const double*)w, (const double*)sigma, (double*)out);
        else
            hipLaunchKernelGGL(assemble_hess_gn_kernel<float>, grid, block, 0, s, cnt, h.w, h.cfg.H, h.cfg.nx, h.nin, map,
                               (const float*)oc, (const float*)tiles, (const float*)w, (const float*)sigma, (float*)out);
    };
    if (hvals) go(nnz, h.d_hess_map.get(), objc, hvals);
    if (hdense) go(nn, h.d_hess_map.get() + (size_t)nnz * h.w, objc + (size_t)nnz * esz, hdense);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

// KKT residuals (nempc_kkt_residual): one wave per problem, four problems per workgroup; the lanes stride over the n
// variables, each entry by kkt_variable_terms (kernels_kkt_impl.h: the band product J' lam straight from the compact tiles,
// sums in double), then over the H nx defects; four wave maxima, and lanes 0..3 store one of them each.
template <typename T>
__global__ __launch_bounds__(256) void kkt_residual_kernel(int B, int H, int nx, int nu, int m, int box, const T* __restrict__ Z,
                                                           const T* __restrict__ grad, const T* __restrict__ g,
                                                           const T* __restrict__ tiles, const T* __restrict__ lam,
                                                           const T* __restrict__ zl, const T* __restrict__ zu,
                                                           const double* __restrict__ lb, const double* __restrict__ ub,
                                                           BoundBind bb, T* __restrict__ r, T* __restrict__ stat) {
    const int b = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (b >= B) return;            // (the whole wave leaves: the reductions below need every lane of theirs)
    const int n = H * (nx + nu), hx = H * nx;
    const size_t on = (size_t)b * n;
    const T* zb = Z + on;
    const T* gradb = grad + on;
    const T* tb = tiles + (size_t)b * hx * (nx + nu);
    const T* lamb = lam + (size_t)b * m;
    const T* zlb = zl ? zl + on : nullptr;
    const T* zub = zu ? zu + on : nullptr;
    double rs = 0.0, rp = 0.0, rc = 0.0, rd = 0.0;
    for (int i = lane; i < n; i += 64) {
        KktTerms k;
        if (bb.B > 0) {     // per-problem bounds bound: problem b against its own effective bounds
            double lo = lb ? lb[i] : -std::numeric_limits<double>::infinity();
            double hi = ub ? ub[i] : std::numeric_limits<double>::infinity();
            bound_bind_intersect<T>(bb, b, i, hx, lo, hi);
            k = kkt_variable_terms_at<T>(i, H, nx, nu, box != 0, zb, gradb, tb, lamb, zlb, zub, lo, hi);
        } else {
            k = kkt_variable_terms<T>(i, H, nx, nu, box != 0, zb, gradb, tb, lamb, zlb, zub, lb, ub);
        }
        if (stat) stat[on + i] = (T)k.s;
        rs = fmax(rs, fabs(k.s)); rp = fmax(rp, k.pfeas); rc = fmax(rc, k.comp); rd = fmax(rd, k.dfeas);
    }
    for (int i = lane; i < hx; i += 64) rp = fmax(rp, fabs((double)g[(size_t)b * m + i]));
    rs = wave_bcast_lane0(wave_max_lane0(rs));
    rp = wave_bcast_lane0(wave_max_lane0(rp));
    rc = wave_bcast_lane0(wave_max_lane0(rc));
    rd = wave_bcast_lane0(wave_max_lane0(rd));
    if (lane < 4) r[(size_t)b * 4 + lane] = (T)(lane == 0 ? rs : (lane == 1 ? rp : (lane == 2 ? rc : rd)));
}

int launch_kkt_residual(Handle& h, int B, const void* Z, const void* grad, const void* g, const void* tiles, const void* lam,
                        const void* zl, const void* zu, const double* lb, const double* ub, void* r, void* stat, hipStream_t s) {
    const dim3 grid((unsigned)((B + 3) / 4)), block(256);
    if (h.cfg.dtype == NEMPC_F64)
        hipLaunchKernelGGL(kkt_residual_kernel<double>, grid, block, 0, s, B, h.cfg.H, h.cfg.nx, h.cfg.nu, h.m, h.box ? 1 : 0,
                           (const double*)Z, (const double*)grad, (const double*)g, (const double*)tiles, (const double*)lam,
                           (const double*)zl, (const double*)zu, lb, ub, h.bbind, (double*)r, (double*)stat);
    else
        hipLaunchKernelGGL(kkt_residual_kernel<float>, grid, block, 0, s, B, h.cfg.H, h.cfg.nx, h.cfg.nu, h.m, h.box ? 1 : 0,
                           (const float*)Z, (const float*)grad, (const float*)g, (const float*)tiles, (const float*)lam,
                           (const float*)zl, (const float*)zu, lb, ub, h.bbind, (float*)r, (float*)stat);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

}  // namespace nempc
