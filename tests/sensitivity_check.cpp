// Host check of csrc/kernels_sens_impl.h (the recursion sens_kernel runs, here with ONE lane and a no-op sync) against a
// plain Gaussian-elimination solve of the dense perturbed KKT system written below.  Stand-alone: includes that header
// and the C++ library only; built by tests/test_sensitivity_reference_cpu.py with AddressSanitizer and
// UndefinedBehaviorSanitizer, every array at its exact size.
//
// Seeded random LQ data, H in {1,2,3,5}, nx, nu in {1,2,3}; per shape four variants: no Sigma; Sigma on the controls; a Sigma
// of 1e8 on one state of the last stage (plus the control Sigma); a deliberately indefinite Quu (verdict 1 expected, no
// output written).  Bound: 1e-10 (1 + |S|inf), S being dz and dlam together.
// The state Sigma is the exception, and the reason is arithmetic, not the code: with Sigma = 1e8 in P the sums
// Quu = .. + B'PB, P <- .. + A'PA + Qux'K and D = A D + B dU add terms of size Sigma that cancel to O(1), and
// dlam = P D multiplies a 1e-8-sized cancelled entry of D by Sigma again, so ANY recursion in double loses about
// 2^-53 Sigma = 1e-8 absolutely (observed here: 3e-10 .. 1e-8, at every H including 1; DESIGN.md "Solution
// sensitivities").  Those cases are held to 64 * 2^-53 * Sigma (1 + |S|inf) -- 64 being a generous count of the
// Sigma-sized terms one result accumulates at nx, nu <= 3 over <= 5 stages -- and their worst figure is printed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "kernels_sens_impl.h"

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

// symmetric positive definite d x d: diag * I + 0.2 sym(N)
std::vector<double> spd(Rng& r, int d, double diag) {
    std::vector<double> m((size_t)d * d);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j <= i; ++j) {
            const double v = 0.2 * r.next();
            m[i * d + j] = m[j * d + i] = v;
        }
    for (int i = 0; i < d; ++i) m[i * d + i] += diag;
    return m;
}

// K x = rhs (N x N, nrhs columns, row-major) by Gaussian elimination with partial pivoting; false when singular
bool gauss(std::vector<double> K, std::vector<double>& X, int N, int nrhs) {
    for (int c = 0; c < N; ++c) {
        int p = c;
        for (int r = c + 1; r < N; ++r)
            if (std::fabs(K[(size_t)r * N + c]) > std::fabs(K[(size_t)p * N + c])) p = r;
        if (K[(size_t)p * N + c] == 0.0) return false;
        if (p != c) {
            for (int j = 0; j < N; ++j) std::swap(K[(size_t)p * N + j], K[(size_t)c * N + j]);
            for (int j = 0; j < nrhs; ++j) std::swap(X[(size_t)p * nrhs + j], X[(size_t)c * nrhs + j]);
        }
        for (int r = c + 1; r < N; ++r) {
            const double f = K[(size_t)r * N + c] / K[(size_t)c * N + c];
            if (f == 0.0) continue;
            for (int j = c; j < N; ++j) K[(size_t)r * N + j] -= f * K[(size_t)c * N + j];
            for (int j = 0; j < nrhs; ++j) X[(size_t)r * nrhs + j] -= f * X[(size_t)c * nrhs + j];
        }
    }
    for (int c = N - 1; c >= 0; --c)
        for (int j = 0; j < nrhs; ++j) {
            double v = X[(size_t)c * nrhs + j];
            for (int k = c + 1; k < N; ++k) v -= K[(size_t)c * N + k] * X[(size_t)k * nrhs + j];
            X[(size_t)c * nrhs + j] = v / K[(size_t)c * N + c];
        }
    return true;
}

}  // namespace

int main() {
    using namespace nempc;
    int cases = 0, failures = 0;
    long entries = 0;
    double worst = 0.0, worst_cancel = 0.0;
    const int Hs[4] = {1, 2, 3, 5};
    auto nosync = [] {};
    for (int hi = 0; hi < 4; ++hi)
        for (int nx = 1; nx <= 3; ++nx)
            for (int nu = 1; nu <= 3; ++nu)
                for (int variant = 0; variant < 4; ++variant) {
                    const int H = Hs[hi], nin = nx + nu, n = H * nin, m = H * nx, N = n + m;
                    Rng rng{(uint64_t)(1000 * H + 100 * nx + 10 * nu + variant)};
                    std::vector<double> tiles((size_t)H * nx * nin), blocks((size_t)H * nin * nin), sig((size_t)n, 0.0);
                    for (double& v : tiles) v = 0.7 * rng.next();
                    for (int t = 0; t < H; ++t)
                        for (int i = 0; i < nin; ++i)
                            for (int j = 0; j <= i; ++j) {
                                const double v = 0.1 * rng.next();
                                blocks[((size_t)t * nin + i) * nin + j] = blocks[((size_t)t * nin + j) * nin + i] = v;
                            }
                    std::vector<double> Qs = spd(rng, nx, 2.0), QTs = spd(rng, nx, 4.0), Rs = spd(rng, nu, 1.0);
                    if (variant == 1 || variant == 2)
                        for (int i = H * nx; i < n; ++i) sig[i] = 5.0 * (1.0 + rng.next());
                    if (variant == 2) sig[(size_t)(H - 1) * nx + (nx - 1)] = 1e8;
                    if (variant == 3)
                        for (int i = 0; i < nu; ++i) Rs[i * nu + i] -= 40.0;
                    // ---- the recursion, one lane
                    const SensLayout L = sens_layout(nx, nu);
                    const double sentinel = -12345.0;
                    std::vector<double> ws((size_t)L.total), Kst((size_t)H * nu * nx), Pst((size_t)H * nx * nx);
                    std::vector<double> dU0((size_t)nu * nx, sentinel), dZ((size_t)n * nx, sentinel), dlam((size_t)m * nx, sentinel),
                        gains((size_t)H * nu * nx, sentinel);
                    const int st = sens_problem<double>(0, 1, nosync, nosync, H, nx, nu, tiles.data(), blocks.data(), Qs.data(), QTs.data(),
                                                        Rs.data(), sig.data(), ws.data(), Kst.data(), Pst.data(), dU0.data(),
                                                        dZ.data(), dlam.data(), gains.data());
                    ++cases;
                    if (variant == 3) {
                        bool untouched = true;
                        for (double v : dZ) untouched = untouched && v == sentinel;
                        for (double v : dU0) untouched = untouched && v == sentinel;
                        if (st != 1 || !untouched) {
                            ++failures;
                            std::printf("FAIL H=%d nx=%d nu=%d indefinite: verdict %d, outputs untouched %d\n", H, nx, nu, st, (int)untouched);
                        }
                        ++entries;
                        continue;
                    }
                    if (st != 0) {
                        ++failures;
                        std::printf("FAIL H=%d nx=%d nu=%d variant=%d: verdict %d\n", H, nx, nu, variant, st);
                        continue;
                    }
                    // ---- the dense system: unknowns [x_0 .. x_{H-1} | u_0 .. u_{H-1} | lam_0 .. lam_{H-1}], nx right-hand sides
                    std::vector<double> K((size_t)N * N, 0.0), X((size_t)N * nx, 0.0);
                    auto W = [&](int t, int i, int j) { return blocks[((size_t)t * nin + i) * nin + j]; };
                    auto T = [&](int t, int i, int j) { return tiles[((size_t)t * nx + i) * nin + j]; };
                    for (int t = 0; t < H; ++t) {
                        const int xo = t * nx, uo = H * nx + t * nu, lo = n + t * nx;
                        for (int i = 0; i < nx; ++i)
                            for (int j = 0; j < nx; ++j) {
                                double v = (t == H - 1 ? QTs : Qs)[i * nx + j];
                                if (t + 1 < H) v += W(t + 1, i, j);
                                if (i == j) v += sig[xo + i];
                                K[(size_t)(xo + i) * N + xo + j] = v;
                            }
                        for (int i = 0; i < nu; ++i)
                            for (int j = 0; j < nu; ++j)
                                K[(size_t)(uo + i) * N + uo + j] = Rs[i * nu + j] + W(t, nx + i, nx + j) + (i == j ? sig[uo + i] : 0.0);
                        if (t > 0)
                            for (int i = 0; i < nu; ++i)
                                for (int j = 0; j < nx; ++j) {
                                    K[(size_t)(uo + i) * N + (t - 1) * nx + j] = W(t, nx + i, j);
                                    K[(size_t)((t - 1) * nx + j) * N + uo + i] = W(t, nx + i, j);
                                }
                        for (int i = 0; i < nx; ++i) {
                            K[(size_t)(lo + i) * N + xo + i] = -1.0;
                            K[(size_t)(xo + i) * N + lo + i] = -1.0;
                            for (int j = 0; j < nu; ++j) {
                                K[(size_t)(lo + i) * N + uo + j] = T(t, i, nx + j);
                                K[(size_t)(uo + j) * N + lo + i] = T(t, i, nx + j);
                            }
                            if (t > 0)
                                for (int j = 0; j < nx; ++j) {
                                    K[(size_t)(lo + i) * N + (t - 1) * nx + j] = T(t, i, j);
                                    K[(size_t)((t - 1) * nx + j) * N + lo + i] = T(t, i, j);
                                }
                        }
                    }
                    for (int j = 0; j < nx; ++j) {
                        for (int i = 0; i < nu; ++i) X[(size_t)(H * nx + i) * nx + j] = -W(0, nx + i, j);
                        for (int i = 0; i < nx; ++i) X[(size_t)(n + i) * nx + j] = -T(0, i, j);
                    }
                    if (!gauss(K, X, N, nx)) {
                        ++failures;
                        std::printf("FAIL H=%d nx=%d nu=%d variant=%d: singular dense system\n", H, nx, nu, variant);
                        continue;
                    }
                    double smax = 1.0, err = 0.0;
                    for (double v : X) smax = std::fmax(smax, std::fabs(v));
                    for (int i = 0; i < n * nx; ++i) err = std::fmax(err, std::fabs(dZ[i] - X[i]));
                    for (int i = 0; i < m * nx; ++i) err = std::fmax(err, std::fabs(dlam[i] - X[(size_t)n * nx + i]));
                    for (int i = 0; i < nu * nx; ++i) {
                        err = std::fmax(err, std::fabs(dU0[i] - X[(size_t)H * nx * nx + i]));
                        if (dU0[i] != gains[i] || dU0[i] != dZ[(size_t)H * nx * nx + i]) err = 1.0;     // the three copies of K_0
                    }
                    // gains: du_t = K_t dx_{t-1} reproduces the control rows
                    for (int t = 1; t < H; ++t)
                        for (int i = 0; i < nu; ++i)
                            for (int j = 0; j < nx; ++j) {
                                double v = 0.0;
                                for (int k = 0; k < nx; ++k) v += gains[((size_t)t * nu + i) * nx + k] * X[(size_t)((t - 1) * nx + k) * nx + j];
                                err = std::fmax(err, std::fabs(v - X[(size_t)(H * nx + t * nu + i) * nx + j]));
                            }
                    entries += (long)(n + m + nu) * nx + (long)(H - 1) * nu * nx;
                    const bool cancels = variant == 2;
                    if (cancels) worst_cancel = std::fmax(worst_cancel, err / smax);
                    else worst = std::fmax(worst, err / smax);
                    if (!(err <= (cancels ? 64.0 * 1.1102230246251565e-16 * 1e8 : 1e-10) * smax)) {
                        ++failures;
                        std::printf("FAIL H=%d nx=%d nu=%d variant=%d: err %.3e, |S|inf %.3e\n", H, nx, nu, variant, err, smax);
                    }
                }
    // Sigma entries: zero multipliers contribute nothing whatever the gap; a non-zero one on a gap <= 0 is flagged
    {
        const double inf = HUGE_VAL;
        bool bad = false;
        const double s0 = sens_sigma_entry(0.25, 2.0, 3.0, -0.75, 0.75, bad);
        if (bad || std::fabs(s0 - (2.0 / 1.0 + 3.0 / 0.5)) > 1e-15) { ++failures; std::printf("FAIL sigma finite\n"); }
        const double s1 = sens_sigma_entry(0.75, 0.0, 0.0, -0.75, 0.75, bad);
        if (bad || s1 != 0.0) { ++failures; std::printf("FAIL sigma zero multiplier at the bound\n"); }
        const double s2 = sens_sigma_entry(0.25, 2.0, 3.0, -inf, inf, bad);
        if (bad || s2 != 0.0) { ++failures; std::printf("FAIL sigma infinite bounds\n"); }
        sens_sigma_entry(0.75, 0.0, 1e-3, -0.75, 0.75, bad);
        if (!bad) { ++failures; std::printf("FAIL sigma undefined not flagged\n"); }
        cases += 4;
        entries += 4;
    }
    std::printf("worst relative error %.3e (state Sigma of 1e8: %.3e)\n", worst, worst_cancel);
    std::printf("%d cases, %ld entries checked, %d failures\n", cases, entries, failures);
    return failures == 0 ? 0 : 1;
}
