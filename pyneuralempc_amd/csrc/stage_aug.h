// Host arithmetic of the stage augmentations nempc_solve runs: the window of a rolling-window model as the stage state
// (solver_roll_impl.h), [x ; u] with the control move as the stage control (nempc_bind_rate, solver_rate_impl.h) and [x ; y]
// with y the value of the linear stage rows (nempc_bind_stage_rows, solver_rows_impl.h; index arithmetic: rows_index.h).  Like
// rate_index.h it includes nothing of HIP and nothing of the library beyond the two layout headers, so that a host program
// checks every table entry by entry (tests/stage_aug_check.cpp, tests/rows_index_check.cpp).  solver_aug.h is the part that
// launches.
//
// The caller's variables are z = [x_1 .. x_H (H nx) | u_0 .. u_{H-1} (H nu)].  What an augmentation states here: the solver's
// stage dimensions, where every caller variable (and every bound it adds) sits in the augmented vector, and the objective
// table over the augmented stage.
#pragma once

#include <cstddef>
#include <vector>

#include "obj_offsets.h"
#include "rate_index.h"

namespace nempc {

// The stage the solver runs on: the handle's own, or an augmentation of it
enum Augmentation { AUG_NONE = 0, AUG_WINDOW = 1, AUG_RATE = 2, AUG_ROWS = 3 };

// ---- stage dimensions of the solver's problem: state, columns of a tile / block, variables, defect rows (nc: rows per stage
// of the rows kind)
struct StageDims { int nx, nin, n, m; };
inline StageDims stage_dims(int kind, int H, int nx, int nu, int w, int nc = 0) {
    const int ns = kind == AUG_WINDOW ? w * nx + (w - 1) * nu : (kind == AUG_RATE ? nx + nu : (kind == AUG_ROWS ? nx + nc : nx));
    return {ns, ns + nu, H * (ns + nu), H * ns};
}

// ---- rolling windows.  Decision variable (index into z) that tile / block column d of step t reads, or -1 when that window
// slot is data (x0 or the bound history).  Column order = the network's input order: w state rows then w control rows,
// oldest first unless rev (model/tensorflow.py:112-130).  For w = 1: [x_{t-1} | u_t].
inline int window_var(int H, int nx, int nu, int w, int rev, int t, int d) {
    const int back = w - 1, wx = w * nx;
    if (d < wx) {
        const int j = d / nx, c = d % nx;
        const int tau = t + (rev ? -j : j - back);   // index into [x0 ; states]
        return tau >= 1 ? (tau - 1) * nx + c : -1;
    }
    d -= wx;
    const int j = d / nu, c = d % nu;
    const int tau = t + (rev ? -j : j - back);
    return tau >= 0 ? H * nx + tau * nu + c : -1;
}

// index tables of a rolling-window model (RollTables, on the host).  x-slot k of s_tau is x_{tau-k} (index into
// [x0 ; states]), u-slot k is u_{tau-1-k}
struct RollTablesHost { std::vector<int> src, src0, prim, isprim, dcol, shift; };
inline RollTablesHost roll_tables(int H, int nx, int nu, int w, int rev) {
    const StageDims d = stage_dims(AUG_WINDOW, H, nx, nu, w);
    const int back = w - 1, wx = w * nx, ns = d.nx, n_r = H * (nx + nu), nin_r = w * (nx + nu);
    auto data_x = [&](int tau, int c) { return tau == 0 ? c : nx + (back + tau) * nx + c; };           // tau <= 0
    auto data_u = [&](int tau, int c) { return nx + back * nx + (back + tau) * nu + c; };               // tau < 0
    RollTablesHost t{std::vector<int>(d.n), std::vector<int>(ns), std::vector<int>(n_r, -1), std::vector<int>(d.n, 0),
                     std::vector<int>(d.nin, -1), std::vector<int>(ns, -1)};
    auto slot_source = [&](int tau_s, int i) {     // entry i of s_{tau_s}: caller variable or -(1 + data index)
        if (i < wx) {
            const int tau = tau_s - i / nx, c = i % nx;
            return tau >= 1 ? (tau - 1) * nx + c : -(1 + data_x(tau, c));
        }
        const int k = (i - wx) / nu, c = (i - wx) % nu, tau = tau_s - 1 - k;
        return tau >= 0 ? H * nx + tau * nu + c : -(1 + data_u(tau, c));
    };
    for (int i = 0; i < ns; ++i) t.src0[i] = slot_source(0, i);
    for (int st = 0; st < H; ++st) {
        for (int i = 0; i < ns; ++i) {
            t.src[st * ns + i] = slot_source(st + 1, i);
            if (i < nx) { t.isprim[st * ns + i] = 1; t.prim[st * nx + i] = st * ns + i; }
        }
        for (int c = 0; c < nu; ++c) {
            const int k = H * ns + st * nu + c;
            t.src[k] = H * nx + st * nu + c; t.isprim[k] = 1; t.prim[H * nx + st * nu + c] = k;
        }
    }
    // window column d of step t (window_var's order) -> column of (s_t, u_t)
    for (int dw = 0; dw < nin_r; ++dw) {
        int col;
        if (dw < wx) {
            const int j = dw / nx, c = dw % nx;
            col = (rev ? j : back - j) * nx + c;                 // x_{t - k}: x-slot k of s_t
        } else {
            const int j = (dw - wx) / nu, c = (dw - wx) % nu, k = rev ? j : back - j;   // u_{t - k}
            col = k == 0 ? ns + c : wx + (k - 1) * nu + c;
        }
        t.dcol[col] = dw;
    }
    // shift rows of s_{t+1}: x-slot k >= 1 copies x-slot k-1 of s_t; u-slot 0 copies u_t, u-slot k copies u-slot k-1
    for (int i = nx; i < ns; ++i) {
        if (i < wx) t.shift[i] = i - nx;
        else { const int k = (i - wx) / nu, c = (i - wx) % nu; t.shift[i] = k == 0 ? ns + c : wx + (k - 1) * nu + c; }
    }
    return t;
}

// ---- bounds.  Slot in the solver's bound vector (StageDims::n) of entry i of the list [the caller's bounds on z (H (nx + nu)) |
// rate: the limits on du_t[j] at t nu + j (H nu); rows: the limits of row (t, k) at t nc + k (H nc)]; every other slot carries
// no bound (the copies inside a window state)
inline std::vector<int> bound_slots(int kind, int H, int nx, int nu, int w, int nc = 0) {
    const int n_r = H * (nx + nu);
    std::vector<int> slot(n_r + (kind == AUG_RATE ? H * nu : (kind == AUG_ROWS ? H * nc : 0)));
    if (kind == AUG_WINDOW) {
        const std::vector<int> prim = roll_tables(H, nx, nu, w, 0).prim;     // (the direction orders tile columns only)
        for (int v = 0; v < n_r; ++v) slot[v] = prim[v];
        return slot;
    }
    if (kind == AUG_ROWS) {      // s_t = [x_t ; y_t], the controls behind the H states: rows_bound_slot / rows_limit_slot of
        const int ns = nx + nc;  // rows_index.h restated (this header's includes are fixed; rows_index_check.cpp holds both together)
        for (int v = 0; v < H * nx; ++v) slot[v] = (v / nx) * ns + v % nx;
        for (int v = H * nx; v < n_r; ++v) slot[v] = H * ns + (v - H * nx);
        for (int k = n_r; k < (int)slot.size(); ++k) slot[k] = ((k - n_r) / nc) * ns + nx + (k - n_r) % nc;
        return slot;
    }
    const RateDims rd = rate_dims(H, nx, nu);
    for (int v = 0; v < n_r; ++v) slot[v] = kind == AUG_RATE ? rate_bound_slot(rd, v) : v;
    for (int k = n_r; k < (int)slot.size(); ++k) slot[k] = rate_limit_slot(rd, (k - n_r) / nu, (k - n_r) % nu);
    return slot;
}

// ---- the objective table over the augmented stage (obj_offsets(H, StageDims::nx, nu)), from the caller's weights: Q, QT
// (nx,nx), R (nu,nu), xref, cx (H,nx), uref, cu (H,nu) and, for the rate kind, S (nu,nu).  Every element is the caller's sum
// in double cast once to T; what is not written is zero.
struct AugObjIn { const double *Q, *R, *QT, *xref, *uref, *cx, *cu, *S; };
template <typename T>
std::vector<T> aug_objective_table(int kind, int H, int nx, int nu, int w, const AugObjIn& in, int nc = 0) {
    const int ns = stage_dims(kind, H, nx, nu, w, nc).nx;
    const ObjOffsets ao = obj_offsets(H, ns, nu);
    std::vector<T> tab((size_t)ao.total, T(0));
    // every kind: the caller's state weights, references and linear costs on the leading (primary) block of s
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j) {
            tab[ao.Q + i * ns + j] = (T)in.Q[i * nx + j];
            tab[ao.Qs + i * ns + j] = (T)(in.Q[i * nx + j] + in.Q[j * nx + i]);
            tab[ao.QT + i * ns + j] = (T)in.QT[i * nx + j];
            tab[ao.QTs + i * ns + j] = (T)(in.QT[i * nx + j] + in.QT[j * nx + i]);
        }
    for (int t = 0; t < H; ++t)
        for (int i = 0; i < nx; ++i) {
            tab[ao.xref + t * ns + i] = (T)in.xref[t * nx + i];
            tab[ao.cx + t * ns + i] = (T)in.cx[t * nx + i];
        }
    // window, rows: the stage control is the caller's -- R, uref, cu as they are (zeros stay on the copies inside s and on the
    // row values y: they cost nothing).
    // rate: the caller's control is the u block of s = [x ; u] -- Q_aug = blkdiag(Q, R), QT_aug = blkdiag(QT, R),
    // [xref ; uref], [cx ; cu] -- and the stage control is the move v: R_aug = S, zero reference and linear cost
    const bool rate = kind == AUG_RATE;
    const double* Rv = rate ? in.S : in.R;
    for (int i = 0; i < nu; ++i)
        for (int j = 0; j < nu; ++j) {
            tab[ao.R + i * nu + j] = (T)Rv[i * nu + j];
            tab[ao.Rs + i * nu + j] = (T)(Rv[i * nu + j] + Rv[j * nu + i]);
            if (!rate) continue;
            const int e = (nx + i) * ns + nx + j;
            tab[ao.Q + e] = tab[ao.QT + e] = (T)in.R[i * nu + j];
            tab[ao.Qs + e] = tab[ao.QTs + e] = (T)(in.R[i * nu + j] + in.R[j * nu + i]);
        }
    for (int t = 0; t < H; ++t)
        for (int i = 0; i < nu; ++i) {
            tab[(rate ? ao.xref + t * ns + nx : ao.uref + t * nu) + i] = (T)in.uref[t * nu + i];
            tab[(rate ? ao.cx + t * ns + nx : ao.cu + t * nu) + i] = (T)in.cu[t * nu + i];
        }
    return tab;
}

}  // namespace nempc
