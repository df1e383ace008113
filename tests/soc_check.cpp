// Host check of csrc/solver_soc_impl.h (the recursion solver_soc_kernel runs: the second-order correction of a rejected full
// step) against a plain dense forward substitution in long double.  Stand-alone: includes that header and the C++ library
// only; built by tests/test_kkt_reference_cpu.py with AddressSanitizer and UndefinedBehaviorSanitizer, every array at its
// exact size (dxbuf: 2 nx).
//
// The recursion runs with ONE lane and a no-op sync, and with 64 simulated lanes: 64 host threads, `sync` a barrier over them
// -- the lanes of the device's wave run in lock step between barriers, host threads in any order, so a missing barrier or a
// half of the ping-pong buffer written while it is still read shows as a wrong number (or, under the sanitizer, not at all:
// the comparison is the check).  nx in {1, 3, 63, 64, 65, 130} x nu in {1, 4} x H in {1, 2, 5} x {double, float}.
// Seeded data: state columns of the tiles uniform in (-0.9, 0.9) / nx (row sums below 0.9: spectral radius below 1), control
// columns, defects and the rejected point uniform in (-1, 1).
// Reference: the H nx square lower-triangular system  dx_t - A_t dx_{t-1} = c_t  written densely and solved row by row in
// long double from the very values the recursion reads.  Bound: 64 u (1 + |dx|inf) H, u = 2^-53 (double) or 2^-24 (float).
// Also checked: every element of the output row is written (it is pre-filled with NaN), the controls are copied unchanged,
// and the 64-lane result equals the one-lane result bit for bit.
#include <pthread.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "solver_soc_impl.h"

namespace {

struct Rng {      // splitmix64 -> uniform in (-1, 1)
    uint64_t s;
    double next() {
        s += 0x9e3779b97f4a7c15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        return (double)(z >> 11) / 9007199254740992.0 * 2.0 - 1.0;
    }
};

template <typename T>
void run_lanes(int nlanes, int nx, int nu, int H, const std::vector<T>& zt, const std::vector<T>& ct, const std::vector<T>& tiles,
               std::vector<T>& zs, std::vector<T>& dxbuf) {
    if (nlanes == 1) {
        nempc::soc_correct_row<T>(0, 1, [] {}, nx, nu, H, zt.data(), ct.data(), tiles.data(), zs.data(), dxbuf.data());
        return;
    }
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, (unsigned)nlanes);
    std::vector<std::thread> th;
    for (int lane = 0; lane < nlanes; ++lane)
        th.emplace_back([&, lane] {
            nempc::soc_correct_row<T>(lane, nlanes, [&bar] { pthread_barrier_wait(&bar); }, nx, nu, H, zt.data(), ct.data(),
                                      tiles.data(), zs.data(), dxbuf.data());
        });
    for (auto& t : th) t.join();
    pthread_barrier_destroy(&bar);
}

template <typename T>
int check(int nx, int nu, int H, uint64_t seed, long& entries, double& worst) {
    const int nin = nx + nu, n = H * nin, hx = H * nx;
    const long double u = sizeof(T) == 8 ? std::ldexp(1.0L, -53) : std::ldexp(1.0L, -24);
    Rng r{seed};
    std::vector<T> tiles((size_t)H * nx * nin), ct((size_t)hx), zt((size_t)n);
    for (int t = 0; t < H; ++t)
        for (int i = 0; i < nx; ++i)
            for (int j = 0; j < nin; ++j) tiles[((size_t)t * nx + i) * nin + j] = (T)(j < nx ? 0.9 * r.next() / nx : r.next());
    for (auto& v : ct) v = (T)r.next();
    for (auto& v : zt) v = (T)r.next();
    // dense reference: row (t, i) of  M dx = c,  M = I - [A_t at block (t, t-1)],  by forward substitution
    std::vector<long double> M((size_t)hx * hx, 0.0L), dx((size_t)hx);
    for (int t = 0; t < H; ++t)
        for (int i = 0; i < nx; ++i) {
            M[((size_t)t * nx + i) * hx + t * nx + i] = 1.0L;
            if (t > 0)
                for (int e = 0; e < nx; ++e) M[((size_t)t * nx + i) * hx + (t - 1) * nx + e] = -(long double)tiles[((size_t)t * nx + i) * nin + e];
        }
    long double dxinf = 0.0L;
    for (int row = 0; row < hx; ++row) {
        long double v = (long double)ct[row];
        for (int k = 0; k < row; ++k) v -= M[(size_t)row * hx + k] * dx[k];
        dx[row] = v / M[(size_t)row * hx + row];
        dxinf = std::fmax(dxinf, std::fabs(dx[row]));
    }
    const long double bound = 64.0L * u * (1.0L + dxinf) * H;
    int failures = 0;
    std::vector<T> first;
    for (int nlanes : {1, 64}) {
        std::vector<T> zs((size_t)n, std::numeric_limits<T>::quiet_NaN()), dxbuf((size_t)2 * nx, std::numeric_limits<T>::quiet_NaN());
        run_lanes<T>(nlanes, nx, nu, H, zt, ct, tiles, zs, dxbuf);
        int bad = 0;
        for (int i = 0; i < n; ++i) {
            if (!(zs[i] == zs[i])) { ++bad; continue; }                          // never written
            if (i >= hx) { bad += zs[i] != zt[i]; continue; }                   // a control: copied unchanged
            const long double e = std::fabs((long double)zs[i] - ((long double)zt[i] + dx[i]));
            worst = std::fmax(worst, (double)(e / bound));
            bad += !(e <= bound);
        }
        entries += n;
        if (nlanes == 1) first = zs;
        else bad += std::memcmp(first.data(), zs.data(), (size_t)n * sizeof(T)) != 0;   // lanes change nothing, bit for bit
        if (bad) {
            std::printf("FAIL %s nx=%d nu=%d H=%d lanes=%d: %d bad entries (bound %.3Le, |dx|inf %.3Lg)\n", sizeof(T) == 8 ? "double" : "float",
                        nx, nu, H, nlanes, bad, bound, dxinf);
            ++failures;
        }
    }
    return failures;
}

}  // namespace

int main() {
    int cases = 0, failures = 0;
    long entries = 0;
    double worst64 = 0.0, worst32 = 0.0;
    uint64_t seed = 1;
    for (int nx : {1, 3, 63, 64, 65, 130})
        for (int nu : {1, 4})
            for (int H : {1, 2, 5}) {
                failures += check<double>(nx, nu, H, ++seed, entries, worst64);
                failures += check<float>(nx, nu, H, ++seed, entries, worst32);
                cases += 4;        // two precisions x {1, 64} lanes
            }
    std::printf("largest error / bound: double %.3f, float %.3f\n", worst64, worst32);
    std::printf("%d cases, %ld entries checked, %d failures\n", cases, entries, failures);
    return failures ? 1 : 0;
}
