// Batched solver, compaction of the unconverged problems to the front of the batch, and the scatter of the results
// back to the caller's order.  Included by solver.hip only.
#pragma once

namespace nempc {

namespace {

// ---- compaction of the unconverged problems (the lock-step batch would otherwise launch every kernel B wide for a
// handful of stragglers).  One workgroup computes the stable partition of slots [0, Bact): perm[new slot] = old slot,
// unconverged first; the rows of every per-problem array that lives across iterations are then gathered into the
// second buffer set.
__global__ __launch_bounds__(1024) void solver_partition_kernel(int Bact, const int* __restrict__ status,
                                                                int* __restrict__ perm, int* __restrict__ count) {
    __shared__ int s_cnt[1024];
    __shared__ int s_tot;
    const int tid = threadIdx.x;
    const int per = (Bact + 1023) / 1024;
    const int lo = tid * per, hi = min(Bact, lo + per);
    int c = 0;
    for (int b = lo; b < hi; ++b) c += status[b] < 0 ? 1 : 0;
    s_cnt[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 1024; ++i) { const int v = s_cnt[i]; s_cnt[i] = run; run += v; }
        s_tot = run;
        *count = run;
    }
    __syncthreads();
    int pa = s_cnt[tid], pi = s_tot + (lo - s_cnt[tid]);     // next active / inactive slot of this thread's range
    for (int b = lo; b < hi; ++b) {
        if (status[b] < 0) perm[pa++] = b; else perm[pi++] = b;
    }
}

struct CompactArrays {   // (src, dst, elements per problem, bytes per element); up to 14 arrays
    const void* src[14];
    void* dst[14];
    int per[14];
    int esz[14];
    int n;
};

__global__ __launch_bounds__(256) void solver_gather_kernel(int Bact, const int* __restrict__ perm, CompactArrays ca) {
    const int slot = blockIdx.x;
    if (slot >= Bact) return;
    const int from = perm[slot];
    for (int k = 0; k < ca.n; ++k) {
        const int words = ca.per[k] * ca.esz[k] / 4;          // every array is a multiple of 4 bytes per problem
        const unsigned* s = (const unsigned*)ca.src[k] + (size_t)from * words;
        unsigned* d = (unsigned*)ca.dst[k] + (size_t)slot * words;
        for (int i = threadIdx.x; i < words; i += 256) d[i] = s[i];
    }
}

// results back in the caller's order: Z_out[orig[slot]] = Z[slot]; unfinished problems are FAIL (1)
template <typename T>
__global__ __launch_bounds__(256) void solver_scatter_kernel(int B, int n, const T* __restrict__ Zc,
                                                             const int* __restrict__ status_c,
                                                             const int* __restrict__ orig,
                                                             const int* __restrict__ iters_c, T* __restrict__ Zout,
                                                             int* __restrict__ status_out, int* __restrict__ iters_out) {
    const int slot = blockIdx.x;
    if (slot >= B) return;
    const int o = orig[slot];
    for (int i = threadIdx.x; i < n; i += 256) Zout[(size_t)o * n + i] = Zc[(size_t)slot * n + i];
    if (threadIdx.x == 0) {
        status_out[o] = status_c[slot] == 0 ? 0 : 1;
        if (iters_out) iters_out[o] = iters_c[slot];
    }
}

// ... and the multipliers the returned iterates carry (nempc_solve_duals), a sibling launch of the scatter above: the defect
// multipliers (zeros on box rows: those limits are bounds here), the bound multipliers -- the carried ones, or mu / slack
// with the problem's final mu under the primal barrier -- and exact zeros on infinite bounds.  Each output may be null.
template <typename T>
__global__ __launch_bounds__(256) void solver_scatter_duals_kernel(int B, int n, int m, int hx, const T* __restrict__ Zc,
                                                                   const T* __restrict__ lamc, const T* __restrict__ zlc,
                                                                   const T* __restrict__ zuc, const T* __restrict__ muc,
                                                                   const T* __restrict__ lb, const T* __restrict__ ub,
                                                                   const int* __restrict__ orig, int bstride, int primal_barrier,
                                                                   T* __restrict__ lam_out, T* __restrict__ zl_out,
                                                                   T* __restrict__ zu_out) {
    const int slot = blockIdx.x;
    if (slot >= B) return;
    const int o = orig[slot];
    if (lam_out)
        for (int i = threadIdx.x; i < m; i += 256) lam_out[(size_t)o * m + i] = i < hx ? lamc[(size_t)slot * m + i] : T(0);
    if (!zl_out && !zu_out) return;
    const T mu = muc[slot];
    for (int i = threadIdx.x; i < n; i += 256) {
        const size_t k = (size_t)slot * n + i;
        const T lo = lb[(size_t)o * bstride + i], hi = ub[(size_t)o * bstride + i];
        const bool flo = lo > -std::numeric_limits<T>::max(), fhi = hi < std::numeric_limits<T>::max();
        T vl = T(0), vu = T(0);
        if (primal_barrier) {
            const T z = Zc[k];
            if (flo && mu > T(0)) vl = mu / (z - lo);
            if (fhi && mu > T(0)) vu = mu / (hi - z);
        } else {
            if (flo) vl = zlc[k];
            if (fhi) vu = zuc[k];
        }
        if (zl_out) zl_out[(size_t)o * n + i] = vl;
        if (zu_out) zu_out[(size_t)o * n + i] = vu;
    }
}

}  // namespace

}  // namespace nempc
