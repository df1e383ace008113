// Host check of csrc/rows_index.h (the index arithmetic of the linear stage rows: solver_rows_impl.h, StageAug<T>) and of the
// AUG_ROWS branches of csrc/stage_aug.h against a brute-force restatement.  Stand-alone: includes those two headers (and what
// stage_aug.h includes: the layout headers) and the C++ library only; built by tests/test_stage_rows_cpu.py with AddressSanitizer
// and UndefinedBehaviorSanitizer.
//
// The restatement writes the augmented vector down as a list of labelled entries, in the order the header's comment gives
// (s_0 .. s_{H-1}, each [x_t ; y_t], then u_0 .. u_{H-1}), the caller's vector likewise ([x_0 .. x_{H-1} | u_0 .. u_{H-1}], x_t
// being row t of the state block), the columns of a stage (s_{t-1}, u_t) and of the handle's tile [x | u], and looks every
// entry up by its label.  Every function of the header is compared with that, entry by entry, and every table built from it
// is filled into a vector of its exact size (so that an index out of range is the sanitizer's to report).  Also checked: the
// stage dimensions handed to the LQ plan, that the slots form a permutation of the augmented vector, where rlo / rhi land for
// both forms of the limit arrays, bound_slots(AUG_ROWS) and the objective table over the augmented stage (the caller's value
// and gradient on x and u, nothing on y).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rows_index.h"
#include "stage_aug.h"

namespace {

using namespace nempc;

struct Label { char kind; int t, i; };      // 'x': x_t[i], 'y': y_t[i], 'u': u_t[i]
bool same(const Label& a, const Label& b) { return a.kind == b.kind && a.t == b.t && a.i == b.i; }

long checked = 0, failures = 0;
void expect(bool ok, const char* what, int a, int b, int c) {
    ++checked;
    if (!ok) { ++failures; std::printf("FAIL %s at (%d, %d, %d)\n", what, a, b, c); }
}
bool close(double a, double b) { return std::fabs(a - b) <= 1e-12 * (1.0 + std::fabs(a) + std::fabs(b)); }

unsigned long long rng_state = 88172645463325252ull;
double rnd() {      // xorshift, in (-1, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state % 2000001ull) / 1000000.0 - 1.0;
}
std::vector<double> rvec(int n) { std::vector<double> v((size_t)n); for (double& x : v) x = rnd(); return v; }

// sum_t (x_t - xref_t)' Q_t (x_t - xref_t) + cx_t' x_t + (u_t - uref_t)' R (u_t - uref_t) + cu_t' u_t over z = [states (H,ns) | controls],
// Q_t = QT at the last step; grad: its gradient
double quad_objective(int H, int ns, int nu, const double* Q, const double* QT, const double* R, const double* xref, const double* uref,
                      const double* cx, const double* cu, const std::vector<double>& z, std::vector<double>& grad) {
    grad.assign((size_t)H * (ns + nu), 0.0);
    double f = 0.0;
    for (int t = 0; t < H; ++t) {
        const double* Qt = t == H - 1 ? QT : Q;
        for (int i = 0; i < ns; ++i) {
            const double di = z.at(t * ns + i) - xref[t * ns + i];
            f += cx[t * ns + i] * z.at(t * ns + i);
            grad.at(t * ns + i) += cx[t * ns + i];
            for (int j = 0; j < ns; ++j) {
                const double dj = z.at(t * ns + j) - xref[t * ns + j];
                f += di * Qt[i * ns + j] * dj;
                grad.at(t * ns + i) += (Qt[i * ns + j] + Qt[j * ns + i]) * dj;
            }
        }
        for (int i = 0; i < nu; ++i) {
            const int k = H * ns + t * nu + i;
            const double di = z.at(k) - uref[t * nu + i];
            f += cu[t * nu + i] * z.at(k);
            grad.at(k) += cu[t * nu + i];
            for (int j = 0; j < nu; ++j) {
                const double dj = z.at(H * ns + t * nu + j) - uref[t * nu + j];
                f += di * R[i * nu + j] * dj;
                grad.at(k) += (R[i * nu + j] + R[j * nu + i]) * dj;
            }
        }
    }
    return f;
}

void run(int nx, int nu, int nc, int H) {
    const RowsDims d = rows_dims(H, nx, nu, nc);
    const int ns = nx + nc, n_s = H * (ns + nu), n_r = H * (nx + nu);
    // ---- the stage dimensions the LQ plan is handed
    expect(d.ns == ns && d.nin == ns + nu && d.n_s == n_s && d.m_s == H * ns && d.n_r == n_r && d.H == H && d.nx == nx && d.nu == nu &&
           d.nc == nc, "dims", nx, nu, H);
    const StageDims sd = stage_dims(AUG_ROWS, H, nx, nu, 1, nc), s0 = stage_dims(AUG_NONE, H, nx, nu, 1);
    expect(sd.nx == ns && sd.nin == ns + nu && sd.n == n_s && sd.m == H * ns, "stage_dims rows", nx, nu, H);
    expect(s0.nx == nx && s0.nin == nx + nu && s0.n == n_r && s0.m == H * nx, "stage_dims plain", nx, nu, H);
    // ---- the two vectors, by label
    std::vector<Label> aug, caller;
    for (int t = 0; t < H; ++t) {
        for (int i = 0; i < nx; ++i) aug.push_back({'x', t, i});
        for (int k = 0; k < nc; ++k) aug.push_back({'y', t, k});
    }
    for (int t = 0; t < H; ++t) for (int j = 0; j < nu; ++j) aug.push_back({'u', t, j});
    for (int t = 0; t < H; ++t) for (int i = 0; i < nx; ++i) caller.push_back({'x', t, i});
    for (int t = 0; t < H; ++t) for (int j = 0; j < nu; ++j) caller.push_back({'u', t, j});
    expect((int)aug.size() == n_s && (int)caller.size() == n_r, "sizes", nx, nu, H);
    auto find = [](const std::vector<Label>& v, const Label& l) { for (size_t k = 0; k < v.size(); ++k) if (same(v[k], l)) return (int)k; return -1; };
    // rows_source: every augmented entry
    std::vector<int> src((size_t)n_s);
    for (int k = 0; k < n_s; ++k) {
        src[(size_t)k] = rows_source(d, k);
        const Label& l = aug[(size_t)k];
        const int want = l.kind == 'y' ? -(1 + l.t * nc + l.i) : find(caller, l);
        expect(src[(size_t)k] == want, "rows_source", k, src[(size_t)k], want);
    }
    // the slots: a permutation of the augmented vector
    std::vector<int> hit((size_t)n_s, 0);
    for (int t = 0; t < H; ++t) {
        for (int i = 0; i < nx; ++i) {
            const int k = rows_slot_x(d, t, i);
            expect(k == find(aug, {'x', t, i}), "rows_slot_x", t, i, k);
            if (k >= 0 && k < n_s) ++hit[(size_t)k];
        }
        for (int c = 0; c < nc; ++c) {
            const int k = rows_slot_y(d, t, c);
            expect(k == find(aug, {'y', t, c}), "rows_slot_y", t, c, k);
            expect(rows_limit_slot(d, t, c) == k, "rows_limit_slot", t, c, k);
            expect(rows_limit_entry(d, t, c, 0) == c && rows_limit_entry(d, t, c, 1) == t * nc + c, "rows_limit_entry", t, c, 0);
            if (k >= 0 && k < n_s) ++hit[(size_t)k];
        }
        for (int j = 0; j < nu; ++j) {
            const int k = rows_slot_u(d, t, j);
            expect(k == find(aug, {'u', t, j}), "rows_slot_u", t, j, k);
            if (k >= 0 && k < n_s) ++hit[(size_t)k];
        }
    }
    for (int k = 0; k < n_s; ++k) expect(hit[(size_t)k] == 1, "permutation", k, hit[(size_t)k], 0);
    // rows_bound_slot: the inverse of rows_source on the caller's variables
    std::vector<int> bslot((size_t)n_r);
    for (int v = 0; v < n_r; ++v) {
        bslot[(size_t)v] = rows_bound_slot(d, v);
        expect(bslot[(size_t)v] == find(aug, caller[(size_t)v]), "rows_bound_slot", v, bslot[(size_t)v], 0);
        expect(bslot[(size_t)v] >= 0 && bslot[(size_t)v] < n_s && src[(size_t)bslot[(size_t)v]] == v, "bound slot inverts source", v, 0, 0);
    }
    // the limit arrays in both forms, read as the binding expands them: entry (t, k) of an (H,nc) array / entry k of an (nc) array
    for (int per_stage = 0; per_stage < 2; ++per_stage) {
        std::vector<double> given((size_t)(per_stage ? H * nc : nc)), expanded((size_t)(H * nc));
        for (size_t e = 0; e < given.size(); ++e) given[e] = 100.0 + (double)e;
        for (int t = 0; t < H; ++t)
            for (int k = 0; k < nc; ++k) {
                expanded.at((size_t)(t * nc + k)) = given.at((size_t)rows_limit_entry(d, t, k, per_stage));
                expect(expanded[(size_t)(t * nc + k)] == 100.0 + (per_stage ? t * nc + k : k), "limit expansion", t, k, per_stage);
            }
    }
    // ---- bound_slots(AUG_ROWS): [the caller's bounds (n_r) | the limits (H nc)], every slot of the bound vector written exactly once
    const std::vector<int> bs = bound_slots(AUG_ROWS, H, nx, nu, 1, nc), b0 = bound_slots(AUG_NONE, H, nx, nu, 1);
    expect((int)bs.size() == n_r + H * nc && (int)bs.size() == n_s && (int)b0.size() == n_r, "bound lists", nx, nu, H);
    std::vector<int> bw((size_t)n_s, 0);
    for (int v = 0; v < n_r; ++v) {
        expect(bs.at(v) == find(aug, caller[(size_t)v]), "bound_slots caller", v, bs.at(v), 0);
        expect(b0.at(v) == v, "bound_slots plain", v, b0.at(v), 0);
    }
    for (int t = 0; t < H; ++t)
        for (int k = 0; k < nc; ++k) expect(bs.at(n_r + t * nc + k) == find(aug, {'y', t, k}), "bound_slots limit", t, k, 0);
    for (int k : bs) if (k >= 0 && k < n_s) ++bw[(size_t)k];
    for (int k = 0; k < n_s; ++k) expect(bw[(size_t)k] == 1, "bound vector", k, bw[(size_t)k], 0);
    // ---- columns of a stage (s_{t-1}, u_t) against the handle's [x_{t-1} | u_t]: x on x, u on u, y on nothing
    std::vector<Label> scol, hcol;
    for (int i = 0; i < nx; ++i) scol.push_back({'x', 0, i});
    for (int k = 0; k < nc; ++k) scol.push_back({'y', 0, k});
    for (int j = 0; j < nu; ++j) scol.push_back({'u', 0, j});
    for (int i = 0; i < nx; ++i) hcol.push_back({'x', 0, i});
    for (int j = 0; j < nu; ++j) hcol.push_back({'u', 0, j});
    expect((int)scol.size() == d.nin, "stage columns", nx, nu, H);
    std::vector<int> dcol((size_t)d.nin), reads((size_t)(nx + nu), 0);
    for (int c = 0; c < d.nin; ++c) {
        dcol[(size_t)c] = rows_handle_col(d, c);
        const int want = scol[(size_t)c].kind == 'y' ? -1 : find(hcol, scol[(size_t)c]);
        expect(dcol[(size_t)c] == want && want < nx + nu, "rows_handle_col", c, dcol[(size_t)c], want);
        if (dcol[(size_t)c] >= 0 && dcol[(size_t)c] < nx + nu) ++reads[(size_t)dcol[(size_t)c]];
    }
    for (int c = 0; c < nx + nu; ++c) expect(reads[(size_t)c] == 1, "tile coverage", c, reads[(size_t)c], 0);
    // ---- the objective table over the augmented stage: the caller's value and gradient on x and u whatever y holds, zero on y
    const std::vector<double> Q = rvec(nx * nx), QT = rvec(nx * nx), R = rvec(nu * nu), xref = rvec(H * nx), uref = rvec(H * nu),
                              cx = rvec(H * nx), cu = rvec(H * nu), S = rvec(nu * nu), z = rvec(n_r), yv = rvec(H * nc);
    const AugObjIn in{Q.data(), R.data(), QT.data(), xref.data(), uref.data(), cx.data(), cu.data(), S.data()};
    const std::vector<double> P = aug_objective_table<double>(AUG_ROWS, H, nx, nu, 1, in, nc);
    const ObjOffsets ao = obj_offsets(H, ns, nu);
    expect((int)P.size() == ao.total, "table size", nx, nu, H);
    std::vector<double> za((size_t)n_s), gr, ga;
    for (int k = 0; k < n_s; ++k) za[(size_t)k] = src[(size_t)k] >= 0 ? z.at(src[(size_t)k]) : yv.at(-1 - src[(size_t)k]);
    const double fr = quad_objective(H, nx, nu, Q.data(), QT.data(), R.data(), xref.data(), uref.data(), cx.data(), cu.data(), z, gr);
    const double fa = quad_objective(H, ns, nu, &P.at(ao.Q), &P.at(ao.QT), &P.at(ao.R), &P.at(ao.xref), &P.at(ao.uref), &P.at(ao.cx),
                                     &P.at(ao.cu), za, ga);
    expect(close(fr, fa), "objective value", nx, nu, H);
    for (int k = 0; k < n_s; ++k)
        expect(src[(size_t)k] >= 0 ? close(ga[(size_t)k], gr.at(src[(size_t)k])) : ga[(size_t)k] == 0.0, "objective gradient", k, nx, H);
    // the symmetrised copies, and R as it is (not S)
    for (int i = 0; i < ns; ++i)
        for (int j = 0; j < ns; ++j) {
            expect(P.at(ao.Qs + i * ns + j) == P.at(ao.Q + i * ns + j) + P.at(ao.Q + j * ns + i), "Qs", i, j, 0);
            expect(P.at(ao.QTs + i * ns + j) == P.at(ao.QT + i * ns + j) + P.at(ao.QT + j * ns + i), "QTs", i, j, 0);
            if (i >= nx || j >= nx) expect(P.at(ao.Q + i * ns + j) == 0.0 && P.at(ao.QT + i * ns + j) == 0.0, "y block", i, j, 0);
        }
    for (int i = 0; i < nu; ++i)
        for (int j = 0; j < nu; ++j) {
            expect(P.at(ao.R + i * nu + j) == R[(size_t)(i * nu + j)], "R", i, j, 0);
            expect(P.at(ao.Rs + i * nu + j) == R[(size_t)(i * nu + j)] + R[(size_t)(j * nu + i)], "Rs", i, j, 0);
        }
    // the float table is the double one cast element by element
    const std::vector<float> Pf = aug_objective_table<float>(AUG_ROWS, H, nx, nu, 1, in, nc);
    expect(Pf.size() == P.size(), "float table size", nx, nu, H);
    for (size_t e = 0; e < P.size() && e < Pf.size(); ++e)
        expect(Pf[e] == (float)P[e], "float cast", (int)e, 0, 0);      // (the sums are the caller's in double, cast once)
}

}  // namespace

int main() {
    const int cases[][4] = {{2, 1, 1, 1}, {2, 1, 1, 6}, {6, 3, 2, 4}, {1, 4, 3, 3}, {70, 3, 5, 2}};
    int n = 0;
    for (const auto& c : cases) { run(c[0], c[1], c[2], c[3]); ++n; }
    std::printf("%d cases, %ld entries checked, %ld failures\n", n, checked, failures);
    return failures == 0 ? 0 : 1;
}
