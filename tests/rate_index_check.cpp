// Host check of csrc/rate_index.h (the index arithmetic of the input-rate formulation: solver_rate_impl.h, Solve<T>) against
// a brute-force restatement.  Stand-alone: includes that header and the C++ library only; built by tests/test_rate_cpu.py with
// AddressSanitizer and UndefinedBehaviorSanitizer.
//
// The restatement writes the augmented vector down as a list of labelled entries, in the order the header's comment gives
// (s_0 .. s_{H-1}, each [x_{t+1} ; u_t], then v_0 .. v_{H-1}), the caller's vector likewise ([x_1 .. x_H | u_0 .. u_{H-1}]),
// the columns of a stage (s_{t-1}, v_t) and of the handle's tile [x | u], and looks every entry up by its label.  Every
// function of the header is compared with that, entry by entry, and every table built from it is filled into a vector of its
// exact size (so that an index out of range is the sanitizer's to report).  Also checked: the stage dimensions handed to the
// LQ plan (ns, nu, ns + nu columns, H ns rows, H (ns + nu) variables), that the slots form a permutation of the augmented
// vector, and where dlo / dhi land for both forms of the limit arrays.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rate_index.h"

namespace {

struct Label { char kind; int t, i; };      // 'x': x_{t+1}[i], 'u': u_t[i], 'v': v_t[i]
bool same(const Label& a, const Label& b) { return a.kind == b.kind && a.t == b.t && a.i == b.i; }

long checked = 0, failures = 0;
void expect(bool ok, const char* what, int a, int b, int c) {
    ++checked;
    if (!ok) { ++failures; std::printf("FAIL %s at (%d, %d, %d)\n", what, a, b, c); }
}

void run(int nx, int nu, int H) {
    const nempc::RateDims d = nempc::rate_dims(H, nx, nu);
    // ---- the stage dimensions the LQ plan is handed
    expect(d.ns == nx + nu && d.nin == nx + 2 * nu && d.n_s == H * (nx + 2 * nu) && d.m_s == H * (nx + nu) && d.n_r == H * (nx + nu) &&
           d.H == H && d.nx == nx && d.nu == nu, "dims", nx, nu, H);
    // ---- the two vectors, by label
    std::vector<Label> aug, caller;
    for (int t = 0; t < H; ++t) {
        for (int i = 0; i < nx; ++i) aug.push_back({'x', t, i});
        for (int j = 0; j < nu; ++j) aug.push_back({'u', t, j});
    }
    for (int t = 0; t < H; ++t) for (int j = 0; j < nu; ++j) aug.push_back({'v', t, j});
    for (int t = 0; t < H; ++t) for (int i = 0; i < nx; ++i) caller.push_back({'x', t, i});
    for (int t = 0; t < H; ++t) for (int j = 0; j < nu; ++j) caller.push_back({'u', t, j});
    expect((int)aug.size() == d.n_s && (int)caller.size() == d.n_r, "sizes", nx, nu, H);
    auto find = [](const std::vector<Label>& v, const Label& l) { for (size_t k = 0; k < v.size(); ++k) if (same(v[k], l)) return (int)k; return -1; };
    // rate_source: every augmented entry
    std::vector<int> src((size_t)d.n_s);
    for (int k = 0; k < d.n_s; ++k) {
        src[(size_t)k] = nempc::rate_source(d, k);
        const Label& l = aug[(size_t)k];
        const int want = l.kind == 'v' ? -(1 + l.t * nu + l.i) : find(caller, l);
        expect(src[(size_t)k] == want, "rate_source", k, src[(size_t)k], want);
    }
    // the slots: a permutation of the augmented vector, and rate_bound_slot the inverse of rate_source on the s slots
    std::vector<int> hit((size_t)d.n_s, 0);
    for (int t = 0; t < H; ++t) {
        for (int i = 0; i < nx; ++i) {
            const int k = nempc::rate_slot_x(d, t, i);
            expect(k == find(aug, {'x', t, i}), "rate_slot_x", t, i, k);
            if (k >= 0 && k < d.n_s) ++hit[(size_t)k];
        }
        for (int j = 0; j < nu; ++j) {
            const int k = nempc::rate_slot_u(d, t, j), kv = nempc::rate_slot_v(d, t, j);
            expect(k == find(aug, {'u', t, j}), "rate_slot_u", t, j, k);
            expect(kv == find(aug, {'v', t, j}), "rate_slot_v", t, j, kv);
            expect(nempc::rate_limit_slot(d, t, j) == kv, "rate_limit_slot", t, j, kv);
            expect(nempc::rate_limit_entry(d, t, j, 0) == j && nempc::rate_limit_entry(d, t, j, 1) == t * nu + j, "rate_limit_entry", t, j, 0);
            if (k >= 0 && k < d.n_s) ++hit[(size_t)k];
            if (kv >= 0 && kv < d.n_s) ++hit[(size_t)kv];
        }
    }
    for (int k = 0; k < d.n_s; ++k) expect(hit[(size_t)k] == 1, "permutation", k, hit[(size_t)k], 0);
    std::vector<int> bslot((size_t)d.n_r);
    for (int v = 0; v < d.n_r; ++v) {
        bslot[(size_t)v] = nempc::rate_bound_slot(d, v);
        expect(bslot[(size_t)v] == find(aug, caller[(size_t)v]), "rate_bound_slot", v, bslot[(size_t)v], 0);
        expect(bslot[(size_t)v] >= 0 && bslot[(size_t)v] < H * d.ns && src[(size_t)bslot[(size_t)v]] == v, "bound slot inverts source", v, 0, 0);
    }
    // the bound vector as upload_bounds fills it: every slot written exactly once by a bound or a limit
    std::vector<int> bw((size_t)d.n_s, 0);
    for (int v = 0; v < d.n_r; ++v) ++bw[(size_t)nempc::rate_bound_slot(d, v)];
    for (int t = 0; t < H; ++t) for (int j = 0; j < nu; ++j) ++bw[(size_t)nempc::rate_limit_slot(d, t, j)];
    for (int k = 0; k < d.n_s; ++k) expect(bw[(size_t)k] == 1, "bound vector", k, bw[(size_t)k], 0);
    // the start state [x0 ; u_prev]
    for (int c = 0; c < d.ns; ++c) {
        expect(nempc::rate_start_is_x0(d, c) == (c < nx), "rate_start_is_x0", c, 0, 0);
        expect(nempc::rate_start_entry(d, c) == (c < nx ? c : c - nx), "rate_start_entry", c, 0, 0);
    }
    // ---- columns of a stage (s_{t-1}, v_t) against the handle's [x_{t-1} | u_t]: x on x, u_{t-1} AND v_t on u
    std::vector<Label> scol, hcol;
    for (int i = 0; i < nx; ++i) scol.push_back({'x', 0, i});
    for (int j = 0; j < nu; ++j) scol.push_back({'u', 0, j});
    for (int j = 0; j < nu; ++j) scol.push_back({'v', 0, j});
    for (int i = 0; i < nx; ++i) hcol.push_back({'x', 0, i});
    for (int j = 0; j < nu; ++j) hcol.push_back({'u', 0, j});
    expect((int)scol.size() == d.nin, "stage columns", nx, nu, H);
    std::vector<int> dcol((size_t)d.nin);
    for (int c = 0; c < d.nin; ++c) {
        dcol[(size_t)c] = nempc::rate_handle_col(d, c);
        const Label& l = scol[(size_t)c];
        const int want = find(hcol, {l.kind == 'v' ? 'u' : l.kind, 0, l.i});
        expect(dcol[(size_t)c] == want && want >= 0 && want < nx + nu, "rate_handle_col", c, dcol[(size_t)c], want);
    }
    // every entry of the handle's tile is read by at least one augmented column (the u columns by two)
    std::vector<int> reads((size_t)(nx + nu), 0);
    for (int c = 0; c < d.nin; ++c) ++reads[(size_t)dcol[(size_t)c]];
    for (int c = 0; c < nx + nu; ++c) expect(reads[(size_t)c] == (c < nx ? 1 : 2), "tile coverage", c, reads[(size_t)c], 0);
    // ---- the linear rows  u_{t-1}[j] + v_t[j] - u_t[j]: derivative with respect to every stage column
    std::vector<int> lin((size_t)(nu * d.nin));
    for (int i = nx; i < d.ns; ++i)
        for (int c = 0; c < d.nin; ++c) {
            const Label& l = scol[(size_t)c];
            const int want = (l.kind == 'u' || l.kind == 'v') && l.i == i - nx ? 1 : 0;
            lin[(size_t)((i - nx) * d.nin + c)] = nempc::rate_linear_entry(d, i, c);
            expect(lin[(size_t)((i - nx) * d.nin + c)] == want, "rate_linear_entry", i, c, want);
        }
}

}  // namespace

int main() {
    const int cases[][3] = {{2, 1, 1}, {2, 1, 6}, {6, 3, 4}, {1, 4, 3}, {70, 3, 2}};
    int n = 0;
    for (const auto& c : cases) { run(c[0], c[1], c[2]); ++n; }
    std::printf("%d cases, %ld entries checked, %ld failures\n", n, checked, failures);
    return failures == 0 ? 0 : 1;
}
