// Per-problem, per-stage bounds bound by nempc_bind_bounds (BoundBind, nempc_internal.h): what the binding says about one
// variable of one problem.  Included by solver.hip (the solver's working copy) and kernels_post.hip (the doubles that
// nempc_kkt_residual and nempc_sensitivity read).
#pragma once

#include <limits>

#include "nempc_internal.h"

namespace nempc {

namespace {

// variable i of problem `prob` (z order: H nx states, then H nu controls; hx = H nx): the binding's lower and upper value as
// stored, -inf / +inf where that array is not bound.  Row t of an x array bounds x_t = z[t nx + j], so the element is i
// itself; row t of a u array bounds u_t = z[hx + t nu + j].
template <typename T>
__device__ __forceinline__ void bound_bind_pair(const BoundBind& bb, int prob, int i, int hx, T& lo, T& hi) {
    const bool isx = i < hx;
    const T* pl = (const T*)(isx ? bb.xlb : bb.ulb);
    const T* pu = (const T*)(isx ? bb.xub : bb.uub);
    const size_t at = (size_t)prob * (size_t)(isx ? bb.ld_x : bb.ld_u) + (size_t)(isx ? i : i - hx);
    lo = pl ? pl[at] : -std::numeric_limits<T>::infinity();
    hi = pu ? pu[at] : std::numeric_limits<T>::infinity();
}

// ... intersected into lo / hi in double with +-inf for "no bound" (nempc_kkt_residual, nempc_sensitivity): the solver's
// working copy in the other number convention, so that a solve's result is judged against the bounds it was solved under
template <typename T>
__device__ __forceinline__ void bound_bind_intersect(const BoundBind& bb, int prob, int i, int hx, double& lo, double& hi) {
    T bl, bu;
    bound_bind_pair<T>(bb, prob, i, hx, bl, bu);
    const T big = std::numeric_limits<T>::max();
    if (bl > -big) lo = fmax(lo, (double)bl);
    if (bu < big) hi = fmin(hi, (double)bu);
}

}  // namespace

}  // namespace nempc
