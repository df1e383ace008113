// Host check of csrc/stage_aug.h (the host arithmetic of the solver's stage augmentations: the window of a rolling-window model
// as the state, and [x ; u] with the control move as the control) against restatements that share no index arithmetic with
// it.  Stand-alone: includes that header and the C++ library only; built by tests/test_stage_aug_cpu.py with AddressSanitizer
// and UndefinedBehaviorSanitizer.  Every table is read through std::vector::at, a slot out of range ends the program.
//
// The restatement writes vectors down as lists of labelled entries -- ('x', tau, c) is x_tau[c] with x_0 = x0 and x_tau, tau < 0,
// the bound history; ('u', tau, c) is u_tau[c], tau < 0 the history (window) or u_prev (rate); ('v', t, c) the move
// u_t - u_{t-1} -- and looks entries up by label:
//     caller   [x_1 .. x_H | u_0 .. u_{H-1}]
//     data     window: [x_0 | x_{-(w-1)} .. x_{-1} | u_{-(w-1)} .. u_{-1}]
//     window   [s_1 .. s_H | u_0 .. u_{H-1}],  s_tau = [x_tau, x_{tau-1}, .., x_{tau-w+1} | u_{tau-1}, .., u_{tau-w+1}];
//              primary copies: the leading x of every s, and the control block
//     rate     [s_0 .. s_{H-1} | v_0 .. v_{H-1}],  s_t = [x_{t+1} ; u_t]
//     network input of step t (window): [x_{t-w+1} .. x_t | u_{t-w+1} .. u_t], newest first when rev
// Grid: H in {1, 2, 5}, nx in {1, 2, 3}, nu in {1, 2}, w in {2, 3, 4}, both directions (H = 1, w = 4: every window slot of every
// step is data; nx = 3, nu = 2: a swapped stride shows).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stage_aug.h"

namespace {

using namespace nempc;

struct Label { char kind; int t, i; bool primary; };
bool same(const Label& a, const Label& b) { return a.kind == b.kind && a.t == b.t && a.i == b.i; }
int find(const std::vector<Label>& v, const Label& l) { for (size_t k = 0; k < v.size(); ++k) if (same(v[k], l)) return (int)k; return -1; }
int count(const std::vector<Label>& v, const Label& l) { int n = 0; for (const Label& x : v) n += same(x, l) ? 1 : 0; return n; }

long checked = 0, failures = 0;
void expect(bool ok, const char* what, int a, int b, int c) {
    ++checked;
    if (!ok) { ++failures; if (failures < 40) std::printf("FAIL %s at (%d, %d, %d)\n", what, a, b, c); }
}
bool close(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fmax(std::fabs(a), std::fabs(b)); }

// a small generator of its own (the values only have to be unequal and of order one)
unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
double rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((rng_state >> 11) & 0xfffff) / (double)0x100000 * 2.0 - 1.0 + 0.03125;
}
std::vector<double> rvec(int n) { std::vector<double> v((size_t)n); for (double& x : v) x = rnd(); return v; }

std::vector<Label> caller_labels(int H, int nx, int nu) {
    std::vector<Label> v;
    for (int t = 1; t <= H; ++t) for (int c = 0; c < nx; ++c) v.push_back({'x', t, c, true});
    for (int t = 0; t < H; ++t) for (int c = 0; c < nu; ++c) v.push_back({'u', t, c, true});
    return v;
}
// s_tau of the window form
std::vector<Label> window_state(int tau, int nx, int nu, int w) {
    std::vector<Label> v;
    for (int k = 0; k < w; ++k) for (int c = 0; c < nx; ++c) v.push_back({'x', tau - k, c, k == 0});
    for (int k = 1; k < w; ++k) for (int c = 0; c < nu; ++c) v.push_back({'u', tau - k, c, false});
    return v;
}

// the caller's objective: value and gradient, plain double loops
struct Weights { std::vector<double> Q, R, QT, xref, uref, cx, cu, S; };
double caller_objective(const Weights& W, int H, int nx, int nu, const std::vector<double>& z, std::vector<double>& grad) {
    double f = 0.0;
    grad.assign(z.size(), 0.0);
    for (int t = 0; t < H; ++t) {
        const std::vector<double>& Q = t == H - 1 ? W.QT : W.Q;
        for (int i = 0; i < nx; ++i) {
            for (int j = 0; j < nx; ++j) {
                const double di = z.at(t * nx + i) - W.xref.at(t * nx + i), dj = z.at(t * nx + j) - W.xref.at(t * nx + j);
                f += di * Q.at(i * nx + j) * dj;
                grad.at(t * nx + i) += (Q.at(i * nx + j) + Q.at(j * nx + i)) * dj;
            }
            f += W.cx.at(t * nx + i) * z.at(t * nx + i);
            grad.at(t * nx + i) += W.cx.at(t * nx + i);
        }
        for (int i = 0; i < nu; ++i) {
            const int ui = H * nx + t * nu + i;
            for (int j = 0; j < nu; ++j) {
                const double di = z.at(ui) - W.uref.at(t * nu + i), dj = z.at(H * nx + t * nu + j) - W.uref.at(t * nu + j);
                f += di * W.R.at(i * nu + j) * dj;
                grad.at(ui) += (W.R.at(i * nu + j) + W.R.at(j * nu + i)) * dj;
            }
            f += W.cu.at(t * nu + i) * z.at(ui);
            grad.at(ui) += W.cu.at(t * nu + i);
        }
    }
    return f;
}
// an objective table read the way the kernels read one (objective_row_value): stage dimensions (ns, nu), variables
// [states (H ns) | controls (H nu)]; the value from Q / R / QT, the gradient from Qs / Rs / QTs
double table_objective(const std::vector<double>& P, int H, int ns, int nu, const std::vector<double>& za, std::vector<double>& grad) {
    const ObjOffsets o = obj_offsets(H, ns, nu);
    double f = 0.0;
    grad.assign(za.size(), 0.0);
    for (int t = 0; t < H; ++t) {
        const int Q = t == H - 1 ? o.QT : o.Q, Qs = t == H - 1 ? o.QTs : o.Qs;
        for (int i = 0; i < ns; ++i) {
            for (int j = 0; j < ns; ++j) {
                const double di = za.at(t * ns + i) - P.at(o.xref + t * ns + i), dj = za.at(t * ns + j) - P.at(o.xref + t * ns + j);
                f += di * P.at(Q + i * ns + j) * dj;
                grad.at(t * ns + i) += P.at(Qs + i * ns + j) * dj;
            }
            f += P.at(o.cx + t * ns + i) * za.at(t * ns + i);
            grad.at(t * ns + i) += P.at(o.cx + t * ns + i);
        }
        for (int i = 0; i < nu; ++i) {
            const int ui = H * ns + t * nu + i;
            for (int j = 0; j < nu; ++j) {
                const double di = za.at(ui) - P.at(o.uref + t * nu + i), dj = za.at(H * ns + t * nu + j) - P.at(o.uref + t * nu + j);
                f += di * P.at(o.R + i * nu + j) * dj;
                grad.at(ui) += P.at(o.Rs + i * nu + j) * dj;
            }
            f += P.at(o.cu + t * nu + i) * za.at(ui);
            grad.at(ui) += P.at(o.cu + t * nu + i);
        }
    }
    return f;
}
Weights random_weights(int H, int nx, int nu) {      // non-symmetric Q, R, S, QT != Q, every reference and linear cost non-zero
    return {rvec(nx * nx), rvec(nu * nu), rvec(nx * nx), rvec(H * nx), rvec(H * nu), rvec(H * nx), rvec(H * nu), rvec(nu * nu)};
}
AugObjIn plain(const Weights& W) { return {W.Q.data(), W.R.data(), W.QT.data(), W.xref.data(), W.uref.data(), W.cx.data(), W.cu.data(), W.S.data()}; }

// the fp32 table is the fp64 table cast element by element
void check_cast(int kind, int H, int nx, int nu, int w, const Weights& W, const std::vector<double>& P) {
    const std::vector<float> Pf = aug_objective_table<float>(kind, H, nx, nu, w, plain(W));
    expect(Pf.size() == P.size(), "fp32 table size", kind, H, nx);
    for (size_t k = 0; k < P.size() && k < Pf.size(); ++k) expect(Pf[k] == (float)P[k], "fp32 table entry", kind, (int)k, 0);
}
// a bound list's slots: in range, none written twice
void check_distinct(const std::vector<int>& slot, int n, const char* what) {
    std::vector<int> hit((size_t)n, 0);
    for (size_t i = 0; i < slot.size(); ++i) {
        expect(slot[i] >= 0 && slot[i] < n, what, (int)i, slot[i], n);
        if (slot[i] >= 0 && slot[i] < n) expect(++hit[(size_t)slot[i]] == 1, what, (int)i, slot[i], -1);
    }
}

void run_window(int H, int nx, int nu, int w, int rev) {
    const int back = w - 1, ns = w * nx + back * nu, nin_s = ns + nu, n_s = H * nin_s, n_r = H * (nx + nu), nin_r = w * (nx + nu);
    const StageDims d = stage_dims(AUG_WINDOW, H, nx, nu, w);
    expect(d.nx == ns && d.nin == nin_s && d.n == n_s && d.m == H * ns, "window dims", H, nx, w);
    // ---- the vectors, by label
    const std::vector<Label> caller = caller_labels(H, nx, nu);
    std::vector<Label> data, aug;
    for (int c = 0; c < nx; ++c) data.push_back({'x', 0, c, false});
    for (int r = 0; r < back; ++r) for (int c = 0; c < nx; ++c) data.push_back({'x', r - back, c, false});
    for (int r = 0; r < back; ++r) for (int c = 0; c < nu; ++c) data.push_back({'u', r - back, c, false});
    for (int tau = 1; tau <= H; ++tau) for (const Label& l : window_state(tau, nx, nu, w)) aug.push_back(l);
    for (int t = 0; t < H; ++t) for (int c = 0; c < nu; ++c) aug.push_back({'u', t, c, true});
    expect((int)aug.size() == n_s && (int)caller.size() == n_r, "window sizes", H, nx, w);
    auto source = [&](const Label& l) {      // caller variable, or -(1 + data entry); every label is one or the other
        const int v = find(caller, l), k = find(data, l);
        expect((v >= 0) != (k >= 0), "label is a variable or data", l.kind, l.t, l.i);
        return v >= 0 ? v : -(1 + k);
    };
    const RollTablesHost T = roll_tables(H, nx, nu, w, rev);
    expect((int)T.src.size() == n_s && (int)T.src0.size() == ns && (int)T.prim.size() == n_r && (int)T.isprim.size() == n_s &&
           (int)T.dcol.size() == nin_s && (int)T.shift.size() == ns, "table sizes", H, nx, w);
    // src, isprim: every augmented entry; src0: s_0 is data only
    for (int k = 0; k < n_s; ++k) {
        expect(T.src.at(k) == source(aug[(size_t)k]), "src", k, T.src.at(k), 0);
        expect(T.isprim.at(k) == (aug[(size_t)k].primary ? 1 : 0), "isprim", k, T.isprim.at(k), 0);
    }
    const std::vector<Label> s0 = window_state(0, nx, nu, w);
    for (int i = 0; i < ns; ++i) expect(T.src0.at(i) == source(s0[(size_t)i]) && T.src0.at(i) < 0, "src0", i, T.src0.at(i), 0);
    // prim: the primary copy of every caller variable, injective, consistent with isprim and src
    for (int v = 0; v < n_r; ++v) {
        int want = -1, copies = 0;
        for (int k = 0; k < n_s; ++k) if (same(aug[(size_t)k], caller[(size_t)v]) && aug[(size_t)k].primary) { want = k; ++copies; }
        const int p = T.prim.at(v);
        expect(copies == 1 && p == want, "prim", v, p, want);
        expect(p >= 0 && p < n_s && T.isprim.at(p) == 1 && T.src.at(p) == v, "prim inverts src", v, p, 0);
    }
    check_distinct(T.prim, n_s, "prim is injective");
    // shift: row i >= nx of s_{t+1} copies a column of (s_t, u_t) -- the column that carries the same label
    {
        const int t = w;      // (any step: the labels move with it)
        std::vector<Label> cols = window_state(t, nx, nu, w);
        for (int c = 0; c < nu; ++c) cols.push_back({'u', t, c, true});
        const std::vector<Label> next = window_state(t + 1, nx, nu, w);
        for (int i = 0; i < ns; ++i)
            expect(T.shift.at(i) == (i < nx ? -1 : find(cols, next[(size_t)i])) && (i < nx || count(cols, next[(size_t)i]) == 1), "shift", i, T.shift.at(i), 0);
    }
    // dcol against window_var: the column of (s_t, u_t) that maps to window column d holds the variable window_var names, or data
    std::vector<int> inv((size_t)nin_r, -1);
    for (int c = 0; c < nin_s; ++c) {
        const int dw = T.dcol.at(c);
        expect(dw >= 0 && dw < nin_r, "dcol range", c, dw, 0);
        if (dw >= 0 && dw < nin_r) { expect(inv[(size_t)dw] == -1, "dcol is injective", c, dw, 0); inv[(size_t)dw] = c; }
    }
    for (int t = 0; t < H; ++t) {
        std::vector<Label> cols = window_state(t, nx, nu, w), net;
        for (int c = 0; c < nu; ++c) cols.push_back({'u', t, c, true});
        for (int j = 0; j < w; ++j) for (int c = 0; c < nx; ++c) net.push_back({'x', rev ? t - j : t - back + j, c, false});
        for (int j = 0; j < w; ++j) for (int c = 0; c < nu; ++c) net.push_back({'u', rev ? t - j : t - back + j, c, false});
        for (int dw = 0; dw < nin_r; ++dw) {
            const int c = inv[(size_t)dw], wv = window_var(H, nx, nu, w, rev, t, dw);
            expect(c >= 0, "every window column has a stage column", t, dw, c);
            if (c < 0) continue;
            const int v = find(caller, cols[(size_t)c]);
            expect(same(cols[(size_t)c], net[(size_t)dw]), "dcol: the network's input order", t, dw, c);
            expect(wv == v, "dcol against window_var", t, dw, wv);      // (both -1: data)
        }
    }
    // bound slots: the primary copies
    const std::vector<int> bs = bound_slots(AUG_WINDOW, H, nx, nu, w);
    expect((int)bs.size() == n_r, "window bound list", H, nx, w);
    check_distinct(bs, n_s, "window bound slots");
    for (int v = 0; v < n_r && v < (int)bs.size(); ++v)
        expect(bs[(size_t)v] >= 0 && bs[(size_t)v] < n_s && aug[(size_t)bs[(size_t)v]].primary && same(aug[(size_t)bs[(size_t)v]], caller[(size_t)v]), "window bound slot", v, bs[(size_t)v], 0);
    // ---- the objective table: on the consistent augmented vector (copies equal to their primaries, data in place) its value is
    //      the caller's, its gradient on a primary slot the caller's and zero on a copy
    const Weights W = random_weights(H, nx, nu);
    const std::vector<double> z = rvec(n_r), dat = rvec((int)data.size());
    std::vector<double> za((size_t)n_s), gr, ga;
    for (int k = 0; k < n_s; ++k) { const int sv = source(aug[(size_t)k]); za[(size_t)k] = sv >= 0 ? z.at(sv) : dat.at(-1 - sv); }
    const std::vector<double> P = aug_objective_table<double>(AUG_WINDOW, H, nx, nu, w, plain(W));
    expect((int)P.size() == obj_offsets(H, ns, nu).total, "window table size", H, nx, w);
    const double fr = caller_objective(W, H, nx, nu, z, gr), fa = table_objective(P, H, ns, nu, za, ga);
    expect(close(fr, fa), "window objective value", H, nx, w);
    for (int k = 0; k < n_s; ++k)
        expect(aug[(size_t)k].primary ? close(ga[(size_t)k], gr.at(find(caller, aug[(size_t)k]))) : ga[(size_t)k] == 0.0, "window objective gradient", k, H, w);
    check_cast(AUG_WINDOW, H, nx, nu, w, W, P);
}

void run_rate(int H, int nx, int nu) {
    const int ns = nx + nu, n_s = H * (ns + nu), n_r = H * (nx + nu);
    const StageDims d = stage_dims(AUG_RATE, H, nx, nu, 1), d0 = stage_dims(AUG_NONE, H, nx, nu, 1);
    expect(d.nx == ns && d.nin == ns + nu && d.n == n_s && d.m == H * ns, "rate dims", H, nx, nu);
    expect(d0.nx == nx && d0.nin == nx + nu && d0.n == n_r && d0.m == H * nx, "plain dims", H, nx, nu);
    const std::vector<Label> caller = caller_labels(H, nx, nu);
    std::vector<Label> aug;
    for (int t = 0; t < H; ++t) {
        for (int c = 0; c < nx; ++c) aug.push_back({'x', t + 1, c, true});
        for (int c = 0; c < nu; ++c) aug.push_back({'u', t, c, true});
    }
    for (int t = 0; t < H; ++t) for (int c = 0; c < nu; ++c) aug.push_back({'v', t, c, false});
    // bound slots: the caller's variables on their labels, the limits on exactly the v entries, nothing written twice
    const std::vector<int> bs = bound_slots(AUG_RATE, H, nx, nu, 1), b0 = bound_slots(AUG_NONE, H, nx, nu, 1);
    expect((int)bs.size() == n_r + H * nu && (int)b0.size() == n_r, "bound lists", H, nx, nu);
    check_distinct(bs, n_s, "rate bound slots");
    for (int v = 0; v < n_r; ++v) {
        expect(bs.at(v) == find(aug, caller[(size_t)v]), "rate bound slot", v, bs.at(v), 0);
        expect(b0.at(v) == v, "plain bound slot", v, b0.at(v), 0);
    }
    for (int t = 0; t < H; ++t)
        for (int c = 0; c < nu; ++c) expect(bs.at(n_r + t * nu + c) == find(aug, {'v', t, c, false}), "rate limit slot", t, c, 0);
    int v_hit = 0;
    for (int k = n_r; k < (int)bs.size(); ++k) v_hit += aug.at(bs[(size_t)k]).kind == 'v' ? 1 : 0;
    expect(v_hit == H * nu && (int)bs.size() == n_s, "the limits cover the v entries", H, nx, nu);
    // ---- the objective table: with v_t = u_t - u_{t-1} its value is the caller's plus sum v'Sv, its gradient on the s slots the
    //      caller's
    const Weights W = random_weights(H, nx, nu);
    const std::vector<double> z = rvec(n_r), up = rvec(nu);
    std::vector<double> za((size_t)n_s), gr, ga;
    double pen = 0.0;
    for (int k = 0; k < n_s; ++k) {
        const Label& l = aug[(size_t)k];
        if (l.kind != 'v') { za[(size_t)k] = z.at(find(caller, l)); continue; }
        za[(size_t)k] = z.at(find(caller, {'u', l.t, l.i, true})) - (l.t == 0 ? up.at(l.i) : z.at(find(caller, {'u', l.t - 1, l.i, true})));
    }
    for (int t = 0; t < H; ++t)
        for (int i = 0; i < nu; ++i)
            for (int j = 0; j < nu; ++j) pen += za.at(find(aug, {'v', t, i, false})) * W.S.at(i * nu + j) * za.at(find(aug, {'v', t, j, false}));
    const std::vector<double> P = aug_objective_table<double>(AUG_RATE, H, nx, nu, 1, plain(W));
    expect((int)P.size() == obj_offsets(H, ns, nu).total, "rate table size", H, nx, nu);
    const double fr = caller_objective(W, H, nx, nu, z, gr), fa = table_objective(P, H, ns, nu, za, ga);
    expect(close(fr + pen, fa), "rate objective value", H, nx, nu);
    for (int v = 0; v < n_r; ++v) expect(close(ga.at(find(aug, caller[(size_t)v])), gr[(size_t)v]), "rate objective gradient", v, H, nx);
    for (int t = 0; t < H; ++t)
        for (int i = 0; i < nu; ++i) {
            double want = 0.0;
            for (int j = 0; j < nu; ++j) want += (W.S.at(i * nu + j) + W.S.at(j * nu + i)) * za.at(find(aug, {'v', t, j, false}));
            expect(close(ga.at(find(aug, {'v', t, i, false})), want), "rate objective gradient on v", t, i, H);
        }
    check_cast(AUG_RATE, H, nx, nu, 1, W, P);
}

}  // namespace

int main() {
    int n = 0;
    for (int H : {1, 2, 5})
        for (int nx : {1, 2, 3})
            for (int nu : {1, 2})
                for (int w : {2, 3, 4})
                    for (int rev : {0, 1}) { run_window(H, nx, nu, w, rev); run_rate(H, nx, nu); ++n; }
    std::printf("%d cases, %ld entries checked, %ld failures\n", n, checked, failures);
    return failures == 0 ? 0 : 1;
}
