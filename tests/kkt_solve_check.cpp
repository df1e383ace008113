// Host check of csrc/kernels_kktsolve_impl.h (the recursion kktsolve_kernel runs, here with ONE lane and a no-op sync)
// against a plain Gaussian-elimination solve of the dense KKT system written below, for caller-supplied right-hand
// sides.  Stand-alone: includes that header (and through it kernels_sens_impl.h) and the C++ library only; built by
// tests/test_kkt_solve_reference_cpu.py with AddressSanitizer and UndefinedBehaviorSanitizer, every array at its exact size.
//
// Seeded random LQ data, H in {1,2,3,5}, nx, nu in {1,2,3}, nrhs in {1,3}; per shape four variants: no Sigma; Sigma on the
// controls; a Sigma of 1e8 on one state of the last stage (plus the control Sigma); a deliberately indefinite Quu (verdict
// 1 expected, no output written).  Right-hand sides rz, rg uniform in (-1, 1); rg is null in the nrhs = 1 runs of variant 0
// (zeros in the dense system).  Checked: v, w and gx0 = -(W_ux,0' v_u[0] + A_0' w_0) from the dense solution.
// Bound: 1e-10 (1 + |[v ; w]|inf).  The state Sigma is the exception, for the reason tests/sensitivity_check.cpp gives for
// its own: with Sigma = 1e8 in P the sums that form Quu, P and the propagated state add terms of size Sigma that cancel to
// O(1), and w = P v_x - p multiplies a 1e-8-sized cancelled entry by Sigma again, so ANY recursion in double loses about
// 2^-53 Sigma = 1e-8 absolutely.  Those cases are held to 64 * 2^-53 * Sigma (1 + |[v ; w]|inf), as there, and their worst
// figure is printed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "kernels_kktsolve_impl.h"

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
    const int Rn[2] = {1, 3};
    auto nosync = [] {};
    for (int hi = 0; hi < 4; ++hi)
        for (int nx = 1; nx <= 3; ++nx)
            for (int nu = 1; nu <= 3; ++nu)
                for (int ri = 0; ri < 2; ++ri)
                    for (int variant = 0; variant < 4; ++variant) {
                        const int H = Hs[hi], nrhs = Rn[ri], nin = nx + nu, n = H * nin, m = H * nx, N = n + m;
                        Rng rng{(uint64_t)(10000 * H + 1000 * nx + 100 * nu + 10 * nrhs + variant)};
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
                        std::vector<double> rz((size_t)nrhs * n), rg((size_t)nrhs * m);
                        for (double& v : rz) v = rng.next();
                        for (double& v : rg) v = rng.next();
                        const bool null_rg = variant == 0 && nrhs == 1;
                        if (null_rg) rg.assign(rg.size(), 0.0);
                        // ---- the recursion, one lane
                        const SensLayout L = sens_layout(nx, nu);
                        const KktSolveLayout A = kktsolve_layout(H, nx, nu, nrhs);
                        const double sentinel = -12345.0;
                        std::vector<double> ws((size_t)L.total), aff((size_t)A.total), Kst((size_t)H * nu * nx), Pst((size_t)H * nx * nx);
                        std::vector<double> v((size_t)nrhs * n, sentinel), w((size_t)nrhs * m, sentinel), gx0((size_t)nrhs * nx, sentinel);
                        const int st = kktsolve_problem<double>(0, 1, nosync, nosync, H, nx, nu, nrhs, tiles.data(), blocks.data(),
                                                                Qs.data(), QTs.data(), Rs.data(), sig.data(), rz.data(),
                                                                null_rg ? nullptr : rg.data(), ws.data(), aff.data(), Kst.data(),
                                                                Pst.data(), v.data(), w.data(), gx0.data());
                        ++cases;
                        if (variant == 3) {
                            bool untouched = true;
                            for (double x : v) untouched = untouched && x == sentinel;
                            for (double x : w) untouched = untouched && x == sentinel;
                            for (double x : gx0) untouched = untouched && x == sentinel;
                            if (st != 1 || !untouched) {
                                ++failures;
                                std::printf("FAIL H=%d nx=%d nu=%d nrhs=%d indefinite: verdict %d, outputs untouched %d\n", H, nx, nu, nrhs, st,
                                            (int)untouched);
                            }
                            ++entries;
                            continue;
                        }
                        if (st != 0) {
                            ++failures;
                            std::printf("FAIL H=%d nx=%d nu=%d nrhs=%d variant=%d: verdict %d\n", H, nx, nu, nrhs, variant, st);
                            continue;
                        }
                        // ---- v and gx0 alone (only P_0 is kept then): the same bits
                        {
                            std::vector<double> ws2((size_t)L.total), aff2((size_t)A.total), Kst2((size_t)H * nu * nx), Pst2((size_t)H * nx * nx);
                            std::vector<double> v2((size_t)nrhs * n, sentinel), g2((size_t)nrhs * nx, sentinel);
                            const int st2 = kktsolve_problem<double>(0, 1, nosync, nosync, H, nx, nu, nrhs, tiles.data(), blocks.data(),
                                                                     Qs.data(), QTs.data(), Rs.data(), sig.data(), rz.data(),
                                                                     null_rg ? nullptr : rg.data(), ws2.data(), aff2.data(), Kst2.data(),
                                                                     Pst2.data(), v2.data(), (double*)nullptr, g2.data());
                            if (st2 != 0 || v2 != v || g2 != gx0) {
                                ++failures;
                                std::printf("FAIL H=%d nx=%d nu=%d nrhs=%d variant=%d: v, gx0 alone differ from the full call\n", H, nx, nu, nrhs, variant);
                            }
                        }
                        // ---- the dense system: unknowns [x_0 .. x_{H-1} | u_0 .. u_{H-1} | w_0 .. w_{H-1}], nrhs columns
                        std::vector<double> K((size_t)N * N, 0.0), X((size_t)N * nrhs, 0.0);
                        auto W = [&](int t, int i, int j) { return blocks[((size_t)t * nin + i) * nin + j]; };
                        auto T = [&](int t, int i, int j) { return tiles[((size_t)t * nx + i) * nin + j]; };
                        for (int t = 0; t < H; ++t) {
                            const int xo = t * nx, uo = H * nx + t * nu, lo = n + t * nx;
                            for (int i = 0; i < nx; ++i)
                                for (int j = 0; j < nx; ++j) {
                                    double x = (t == H - 1 ? QTs : Qs)[i * nx + j];
                                    if (t + 1 < H) x += W(t + 1, i, j);
                                    if (i == j) x += sig[xo + i];
                                    K[(size_t)(xo + i) * N + xo + j] = x;
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
                        for (int c = 0; c < nrhs; ++c) {
                            for (int i = 0; i < n; ++i) X[(size_t)i * nrhs + c] = rz[(size_t)c * n + i];
                            for (int i = 0; i < m; ++i) X[(size_t)(n + i) * nrhs + c] = rg[(size_t)c * m + i];
                        }
                        if (!gauss(K, X, N, nrhs)) {
                            ++failures;
                            std::printf("FAIL H=%d nx=%d nu=%d nrhs=%d variant=%d: singular dense system\n", H, nx, nu, nrhs, variant);
                            continue;
                        }
                        double smax = 1.0, err = 0.0;
                        for (double x : X) smax = std::fmax(smax, std::fabs(x));
                        for (int c = 0; c < nrhs; ++c) {
                            for (int i = 0; i < n; ++i) err = std::fmax(err, std::fabs(v[(size_t)c * n + i] - X[(size_t)i * nrhs + c]));
                            for (int i = 0; i < m; ++i) err = std::fmax(err, std::fabs(w[(size_t)c * m + i] - X[(size_t)(n + i) * nrhs + c]));
                            for (int j = 0; j < nx; ++j) {
                                double g = 0.0;
                                for (int i = 0; i < nu; ++i) g += W(0, nx + i, j) * X[(size_t)(H * nx + i) * nrhs + c];
                                for (int i = 0; i < nx; ++i) g += T(0, i, j) * X[(size_t)(n + i) * nrhs + c];
                                err = std::fmax(err, std::fabs(gx0[(size_t)c * nx + j] + g));
                            }
                        }
                        entries += (long)(n + m + nx) * nrhs;
                        const bool cancels = variant == 2;
                        if (cancels) worst_cancel = std::fmax(worst_cancel, err / smax);
                        else worst = std::fmax(worst, err / smax);
                        if (!(err <= (cancels ? 64.0 * 1.1102230246251565e-16 * 1e8 : 1e-10) * smax)) {
                            ++failures;
                            std::printf("FAIL H=%d nx=%d nu=%d nrhs=%d variant=%d: err %.3e, |[v;w]|inf %.3e\n", H, nx, nu, nrhs, variant, err, smax);
                        }
                    }
    std::printf("worst relative error %.3e (state Sigma of 1e8: %.3e)\n", worst, worst_cancel);
    std::printf("%d cases, %ld entries checked, %d failures\n", cases, entries, failures);
    return failures == 0 ? 0 : 1;
}
