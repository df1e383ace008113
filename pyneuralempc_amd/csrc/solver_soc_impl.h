// Arithmetic of the second-order correction of a rejected full step (solver_soc_kernel, solver_merit_impl.h).  Like
// kernels_kktsolve_impl.h it includes nothing of the library and nothing of HIP, so that a host program runs the very same
// recursion with one lane or with simulated lanes (tests/soc_check.cpp).
//
// States only:  dx_t = A_t dx_{t-1} + c+_t  (dx_{-1} = 0: x0 is data),  zs_x[t] = zt_x[t] + dx_t,  zs_u = zt_u, where
// A_t = dPhi_t / dx_{t-1} are the first nx columns of the iterate's Jacobian tile of stage t (row-major (nx, nx + nu)) and c+
// the defects of the rejected trial point zt.  Any nx: lane `lane` of `nlanes` walks the rows i = lane, lane + nlanes, ...;
// dx_{t-1} lives in `dxbuf` (2 nx elements, ping-pong: a stage reads one half and writes the other, one `sync` per stage).
// Per row the sum runs over e = 0 .. nx-1 in that order, one fma each, from c+_t[i]: what a lane of the one-state-per-lane
// form computed, bit for bit.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEMPC_SOC_HD __host__ __device__
#else
#define NEMPC_SOC_HD
#endif

namespace nempc {

NEMPC_SOC_HD inline float soc_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
NEMPC_SOC_HD inline double soc_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// zt, zs: one problem's point (n = H (nx + nu): H nx states, then H nu controls); ct: its H nx defects; tiles: its H tiles
template <typename T, typename Sync>
NEMPC_SOC_HD inline void soc_correct_row(int lane, int nlanes, Sync sync, int nx, int nu, int H, const T* zt, const T* ct,
                                         const T* tiles, T* zs, T* dxbuf) {
    const int nin = nx + nu, n = H * nin;
    T* prev = dxbuf;
    T* next = dxbuf + nx;
    for (int i = lane; i < nx; i += nlanes) prev[i] = T(0);
    sync();
    for (int t = 0; t < H; ++t) {
        const T* At = tiles + (long)t * nx * nin;          // row i: dPhi_i / d[x_{t-1} | u_t]
        for (int i = lane; i < nx; i += nlanes) {
            T acc = ct[t * nx + i];
            for (int e = 0; e < nx; ++e) acc = soc_fma(At[i * nin + e], prev[e], acc);
            next[i] = acc;
            zs[t * nx + i] = zt[t * nx + i] + acc;
        }
        sync();
        T* sw = prev; prev = next; next = sw;
    }
    for (int i = H * nx + lane; i < n; i += nlanes) zs[i] = zt[i];
}

}  // namespace nempc
