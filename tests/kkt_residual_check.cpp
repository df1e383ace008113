// Stand-alone host check of the KKT residual evaluator's per-variable arithmetic (pyneuralempc_amd/csrc/kernels_kkt_impl.h):
// the function the device kernel calls, compiled for the host with -fsanitize=address,undefined, against a dense triple
// loop (J assembled as a full (m, n) matrix, s = grad f + J' lam - zl + zu).  Every array is allocated at its exact size,
// so a load past a tile, a multiplier row or a bound vector is a sanitizer report.  Shapes: H = 1 (no A_{t+1} term), the
// last stage, n > 64 and n no multiple of 64; with and without box rows; null and non-null bound multipliers; null bound
// vectors; infinite bounds mixed in.  Includes nothing of the library but that header.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "kernels_kkt_impl.h"

namespace {

struct Shape { int nx, nu, H; };

template <typename T>
int check(const Shape& sh, bool box, bool with_mult, int bound_mode, std::mt19937_64& rng, long& entries) {
    // bound_mode 0: lb / ub null; 1: all finite; 2: finite, -inf / +inf mixed
    const int nx = sh.nx, nu = sh.nu, H = sh.H, nin = nx + nu, hx = H * nx, n = H * nin, m = hx + (box ? hx : 0);
    std::normal_distribution<double> N(0.0, 1.0);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<T> z(n), grad(n), tiles((size_t)hx * nin), lam(m), zl(n), zu(n);
    std::vector<double> lb(n), ub(n);
    for (auto& v : z) v = (T)N(rng);
    for (auto& v : grad) v = (T)N(rng);
    for (auto& v : tiles) v = (T)N(rng);
    for (auto& v : lam) v = (T)(3.0 * N(rng));
    for (int i = 0; i < n; ++i) {
        zl[i] = (T)(U(rng) < 0.2 ? -U(rng) : U(rng));          // (some negative: dual infeasibility has to show)
        zu[i] = (T)(U(rng) < 0.2 ? -U(rng) : U(rng));
        lb[i] = (double)z[i] - (U(rng) < 0.2 ? -0.3 : 1.0) * U(rng);     // (some violated)
        ub[i] = (double)z[i] + (U(rng) < 0.2 ? -0.3 : 1.0) * U(rng);
        if (bound_mode == 2 && U(rng) < 0.35) lb[i] = -std::numeric_limits<double>::infinity();
        if (bound_mode == 2 && U(rng) < 0.35) ub[i] = std::numeric_limits<double>::infinity();
    }
    const T* zlp = with_mult ? zl.data() : nullptr;
    const T* zup = with_mult ? zu.data() : nullptr;
    const double* lbp = bound_mode ? lb.data() : nullptr;
    const double* ubp = bound_mode ? ub.data() : nullptr;

    // dense reference: J (m, n) with -I on x_t, the tile of step t on [x_{t-1} | u_t], +I box rows
    std::vector<double> J((size_t)m * n, 0.0);
    for (int t = 0; t < H; ++t)
        for (int k = 0; k < nx; ++k) {
            double* row = J.data() + (size_t)(t * nx + k) * n;
            row[t * nx + k] -= 1.0;
            for (int j = 0; j < nx; ++j)
                if (t > 0) row[(t - 1) * nx + j] += (double)tiles[((size_t)t * nx + k) * nin + j];
            for (int j = 0; j < nu; ++j) row[hx + t * nu + j] += (double)tiles[((size_t)t * nx + k) * nin + nx + j];
        }
    if (box)
        for (int k = 0; k < hx; ++k) J[(size_t)(hx + k) * n + k] = 1.0;

    int bad = 0;
    for (int i = 0; i < n; ++i) {
        const nempc::KktTerms got = nempc::kkt_variable_terms<T>(i, H, nx, nu, box, z.data(), grad.data(), tiles.data(),
                                                                 lam.data(), zlp, zup, lbp, ubp);
        double s = (double)grad[i], mag = std::fabs((double)grad[i]);
        for (int r = 0; r < m; ++r) {
            s += J[(size_t)r * n + i] * (double)lam[r];
            mag += std::fabs(J[(size_t)r * n + i] * (double)lam[r]);
        }
        const bool flo = lbp && std::isfinite(lb[i]), fhi = ubp && std::isfinite(ub[i]);
        const double vl = flo && zlp ? (double)zl[i] : 0.0, vu = fhi && zup ? (double)zu[i] : 0.0;
        s += -vl + vu;
        mag += std::fabs(vl) + std::fabs(vu);
        double pf = 0.0, cp = 0.0, df = 0.0;
        if (flo) {
            pf = std::fmax(pf, lb[i] - (double)z[i]);
            cp = std::fmax(cp, std::fabs(vl * ((double)z[i] - lb[i])));
            df = std::fmax(df, -vl);
        }
        if (fhi) {
            pf = std::fmax(pf, (double)z[i] - ub[i]);
            cp = std::fmax(cp, std::fabs(vu * (ub[i] - (double)z[i])));
            df = std::fmax(df, -vu);
        }
        // both sides sum the same doubles in a different order: a few ulps of the largest partial sum
        const double tol = 64.0 * std::numeric_limits<double>::epsilon() * (1.0 + mag);
        const bool ok = std::fabs(got.s - s) <= tol && got.pfeas == pf && std::fabs(got.comp - cp) <= tol && got.dfeas == df;
        if (!ok) {
            if (bad < 5)
                std::printf("MISMATCH %d/%d/%d box=%d mult=%d bounds=%d i=%d: s %.17g vs %.17g, pfeas %.17g vs %.17g, "
                            "comp %.17g vs %.17g, dfeas %.17g vs %.17g\n", nx, nu, H, (int)box, (int)with_mult, bound_mode, i,
                            got.s, s, got.pfeas, pf, got.comp, cp, got.dfeas, df);
            ++bad;
        }
        ++entries;
    }
    return bad;
}

}  // namespace

int main() {
    const Shape shapes[] = {{2, 1, 1}, {2, 1, 2}, {2, 1, 3}, {3, 2, 7}, {6, 3, 8}, {2, 1, 63}};
    std::mt19937_64 rng(12345);
    long entries = 0;
    int bad = 0, cases = 0;
    for (const Shape& sh : shapes)
        for (int box = 0; box < 2; ++box)
            for (int mult = 0; mult < 2; ++mult)
                for (int bm = 0; bm < 3; ++bm) {
                    bad += check<double>(sh, box != 0, mult != 0, bm, rng, entries);
                    bad += check<float>(sh, box != 0, mult != 0, bm, rng, entries);
                    cases += 2;
                }
    std::printf("%d cases, %ld entries checked, %d failures\n", cases, entries, bad);
    return bad ? 1 : 0;
}
