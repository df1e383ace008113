// Internal declarations shared by the translation units of libnempc.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "dev_buf.h"          // DevBuf: every device allocation a Handle owns
#include "jac_resident.h"
#include "mfma_plan.h"
#include "obj_offsets.h"      // ObjOffsets / obj_offsets: the objective table's layout
#include "post_plan.h"
#include "nempc.h"

namespace nempc {

// codes of the dense / sparse assembly maps: >= 0 is an index into one problem's tile array
// (H, nx, w*(nx+nu)); negative codes are constants
constexpr int32_t MAP_ZERO = -1;
constexpr int32_t MAP_MINUS_ONE = -2;
constexpr int32_t MAP_PLUS_ONE = -3;

void set_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what);

// Environment knobs (A/B switches, diagnostics): the only readers of the environment in the library.  A call reads the
// variable afresh; a knob that is read once per process keeps the value in a `static const` at its (one) site.
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline double env_double(const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; }
inline bool env_enabled(const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); }   // on unless it parses to 0
inline bool env_set(const char* name) { return getenv(name) != nullptr; }                                   // set at all, to anything

#define NEMPC_HIP(call)                                            \
    do {                                                           \
        hipError_t _e = (call);                                    \
        if (_e != hipSuccess) return ::nempc::hip_fail(_e, #call); \
    } while (0)

// How one (problem, step) row reads its network inputs: plain models read [x_{t-1} | u_t]; rolling-window models
// (model/tensorflow.py:112-130 rolling_input) read the last w states and controls, reaching into x0 and the bound
// history before the horizon.  Tile / block column d indexes the window in the network's input order.
struct RowGather {
    int H, nx, nu, n;       // n = H*(nx+nu)
    int w, rev;             // window length, newest-first flag
    int xcur;               // tile column of the current state x_{t-1}, component 0 (where DISCRET adds its identity)
    unsigned inv_nx, inv_nu; // ceil(2^32 / nx), ceil(2^32 / nu) (0 for a divisor of 1): d / nx == umulhi(d, inv_nx), exact while d * nx < 2^32
    const void* hx;         // (B, w-1, nx) states before x0, oldest first
    const void* hu;         // (B, w-1, nu) controls before u_0
};

// value of window column d (< w*(nx+nu)) of row (b,t); z = this problem's decision vector
template <typename T>
__device__ __forceinline__ T gather_input(const RowGather& gk, const T* __restrict__ z, const T* __restrict__ X0,
                                          int b, int t, int d) {
    const int nx = gk.nx, nu = gk.nu;
    if (gk.w == 1) {
        if (d < nx) return t == 0 ? X0[(size_t)b * nx + d] : z[(t - 1) * nx + d];
        return z[gk.H * nx + t * nu + (d - nx)];
    }
    const int wx = gk.w * nx, back = gk.w - 1;
    if (d < wx) {
        const int j = nx == 1 ? d : (int)__umulhi((unsigned)d, gk.inv_nx), c = d - j * nx;
        const int tau = t + (gk.rev ? -j : j - back);   // index into [x0 ; states]: 0 is x0
        if (tau >= 1) return z[(tau - 1) * nx + c];
        if (tau == 0) return X0[(size_t)b * nx + c];
        return static_cast<const T*>(gk.hx)[((size_t)b * back + (back + tau)) * nx + c];
    }
    d -= wx;
    const int j = nu == 1 ? d : (int)__umulhi((unsigned)d, gk.inv_nu), c = d - j * nu;
    const int tau = t + (gk.rev ? -j : j - back);
    if (tau >= 0) return z[gk.H * nx + tau * nu + c];
    return static_cast<const T*>(gk.hu)[((size_t)b * back + (back + tau)) * nu + c];
}

// ... and where that value lives (the same case analysis, as an address: a caller with several columns to fetch forms all the
// addresses first and then has all the loads in flight together)
template <typename T>
__device__ __forceinline__ const T* gather_input_ptr(const RowGather& gk, const T* __restrict__ z, const T* __restrict__ X0,
                                                     int b, int t, int d) {
    const int nx = gk.nx, nu = gk.nu;
    if (gk.w == 1) {
        if (d < nx) return t == 0 ? X0 + ((size_t)b * nx + d) : z + ((t - 1) * nx + d);
        return z + (gk.H * nx + t * nu + (d - nx));
    }
    const int wx = gk.w * nx, back = gk.w - 1;
    if (d < wx) {
        const int j = nx == 1 ? d : (int)__umulhi((unsigned)d, gk.inv_nx), c = d - j * nx;
        const int tau = t + (gk.rev ? -j : j - back);   // index into [x0 ; states]: 0 is x0
        if (tau >= 1) return z + ((tau - 1) * nx + c);
        if (tau == 0) return X0 + ((size_t)b * nx + c);
        return static_cast<const T*>(gk.hx) + (((size_t)b * back + (back + tau)) * nx + c);
    }
    d -= wx;
    const int j = nu == 1 ? d : (int)__umulhi((unsigned)d, gk.inv_nu), c = d - j * nu;
    const int tau = t + (gk.rev ? -j : j - back);
    if (tau >= 0) return z + (gk.H * nx + tau * nu + c);
    return static_cast<const T*>(gk.hu) + (((size_t)b * back + (back + tau)) * nu + c);
}

// MFMA-packed network (built by nempc_set_weights when the MFMA row kernel is selected)
struct MfmaNet {
    int wp = 0;        // padded hidden width (multiple of 16): 32 | 64 | 128
    int nh = 0;        // hidden layers
    int kin = 0;       // padded input width (multiple of 4)
    int ldw = 0;       // leading dimension (elements) of every packed matrix
    DevBuf<> blob;     // device, dtype T; see kernels_mfma.hip for the layout
};

struct ObjHost {   // host copy of the objective parameters (doubles), re-uploaded whenever one of them changes
    std::vector<double> Q, R, xref, uref, cx, cu;
};

// Per-problem tracking data bound by nempc_bind_tracking: base pointers (dtype of the handle; null = the shared table's
// array) and the element strides from one problem's block to the next.  B = problems covered, 0 = nothing bound.
struct TrackBind {
    const void *xref = nullptr, *uref = nullptr, *cx = nullptr, *cu = nullptr;
    long long ld_x = 0, ld_u = 0;
    int B = 0;
    bool on() const { return xref || uref || cx || cu; }
};

// Per-problem, per-stage variable bounds bound by nempc_bind_bounds: base pointers (dtype of the handle; null = adds
// nothing) and the element strides from one problem's block to the next.  B = problems covered, 0 = nothing bound.
struct BoundBind {
    const void *xlb = nullptr, *xub = nullptr, *ulb = nullptr, *uub = nullptr;
    long long ld_x = 0, ld_u = 0;
    int B = 0;
    bool on() const { return xlb || xub || ulb || uub; }
};

// Input-rate penalty and rate limits bound by nempc_bind_rate: host copies of the weight and of the limits (expanded to
// (H,nu), +-inf = no limit) and the device pointer of the controls applied before each problem's first step.  B = problems
// u_prev covers, 0 = nothing bound.
struct RateBind {
    const void* u_prev = nullptr;
    int B = 0;
    std::vector<double> S, dlo, dhi;      // (nu,nu) (zeros when no penalty was given), (H,nu), (H,nu)
    bool on() const { return u_prev != nullptr; }
};

// Linear stage inequality rows bound by nempc_bind_stage_rows: host copies of C = [Cx | Cu] (nc, nx + nu) and of the limits
// (expanded to (H,nc), +-inf = no limit).  The device copy of C, in the handle's dtype, is Handle::d_rows_C.  nc = 0: nothing bound.
struct RowsBind {
    int nc = 0;
    std::vector<double> C, lo, hi;
    bool on() const { return nc > 0; }
};

// Device memory: every allocation the handle owns is a DevBuf member (dev_buf.h) and goes with the handle; a new workspace is
// one more member and nothing else.  What a caller bound (d_extra, d_hist_*, the bindings, jac_resident's entries) stays a
// raw pointer.  solver_ws and comm are opaque to everyone but their units, which free them (solver_free, comm_free).
struct Handle {
    ~Handle();                   // (nempc_api.hip: solver_free, comm_free; the members free themselves)
    nempc_config cfg{};
    int num_cus = 256;           // compute units of cfg.device (nempc_create)
    size_t lds_limit = 65536;    // LDS a workgroup of cfg.device may ask for (hipDeviceProp_t::sharedMemPerBlock, nempc_create)
    int n = 0, m = 0, nl = 0;
    int nin = 0;                 // tile width = decision inputs one row's network reads: w*(nx+nu)
    int ne = 0;                  // extra network inputs (tvp + p); the network's input width is nin + ne
    const void* d_extra = nullptr;  // bound by nempc_bind_extra, (B,H,ne)
    int extra_B = 0;                // problems the bound extras cover
    int hist_B = 0;                 // problems the bound history covers
    int w = 1, rev = 0;          // rolling window (1 = plain model), newest-first flag
    const void* d_hist_x = nullptr;  // bound by nempc_bind_history
    const void* d_hist_u = nullptr;
    TrackBind track;             // bound by nempc_bind_tracking
    BoundBind bbind;             // bound by nempc_bind_bounds
    RateBind rate;               // bound by nempc_bind_rate
    RowsBind rows;               // bound by nempc_bind_stage_rows
    DevBuf<> d_rows_C;           // ... and its C on the device, dtype T (nc, nx + nu)
    RowGather gather() const {
        RowGather gk;
        gk.H = cfg.H; gk.nx = cfg.nx; gk.nu = cfg.nu; gk.n = n; gk.w = w; gk.rev = rev;
        gk.xcur = rev ? 0 : (w - 1) * cfg.nx;
        gk.inv_nx = cfg.nx == 1 ? 0u : (unsigned)(((1ull << 32) + cfg.nx - 1) / (unsigned)cfg.nx);
        gk.inv_nu = cfg.nu == 1 ? 0u : (unsigned)(((1ull << 32) + cfg.nu - 1) / (unsigned)cfg.nu);
        gk.hx = d_hist_x; gk.hu = d_hist_u;
        return gk;
    }
    int din[NEMPC_MAX_LAYERS]{}, dout[NEMPC_MAX_LAYERS]{};
    int act[NEMPC_MAX_LAYERS]{};   // NEMPC_ACT_* per layer (cfg.activations)
    double actp[NEMPC_MAX_LAYERS]{};   // alpha of elu / leaky_relu layers (cfg.act_param)
    int mfma_act = -1;             // the one hidden activation when the matrix-core kernels can take the network
                                   // (same non-linear activation on every hidden layer, linear output layer), else -1
    int maxw = 0;
    bool box = false;
    bool have_weights = false;
    bool have_objective = false;
    int variant = NEMPC_KERNEL_VALU;
    size_t esz = 8;

    // network, dtype T on device. W[l] (in,out) row-major; Wt[l] (out,in) row-major
    DevBuf<> d_W[NEMPC_MAX_LAYERS];
    DevBuf<> d_Wt[NEMPC_MAX_LAYERS];
    DevBuf<> d_b[NEMPC_MAX_LAYERS];
    MfmaNet mfma;

    // objective, dtype T: Q, Qs=Q+Q^T, R, Rs, xref, uref, cx, cu, QT, QTs (one allocation) + Hessian constants
    DevBuf<> d_obj;              // (a change of values overwrites it in place)
    bool hess_maps_built = false;   // the Hessian structure / maps depend on the shape only: built once per handle
    ObjHost obj_host;            // last nempc_set_objective arguments (defaults filled in)
    std::vector<double> obj_QT;  // terminal state weight (host copy; empty = same as Q), nempc_set_terminal_weight
    // bounds (host)
    std::vector<double> box_lo, box_hi;

    // structure (host) + assembly maps (device)
    std::vector<int32_t> jac_rows, jac_cols, hess_rows, hess_cols;
    DevBuf<int32_t> d_dense_map;      // (m*n)
    DevBuf<int32_t> d_sparse_map;     // (nnz_jac)
    DevBuf<int32_t> d_sparse_pos;     // (nnz_jac) where each structural non-zero sits in one problem's dense matrix: row * n + col
    JacResidentTable jac_resident;    // dense-Jacobian buffers whose structural zeros are in place (nempc_jac_dense_resident)
    DevBuf<int32_t> d_hess_map;       // (nnz_hess + n*n, w) per-row block elements summed into each entry; -1 = none
    DevBuf<int32_t> d_hess_smap;      // plain models: (H*nin*nin) block element -> tril entry (-1 none), then the entries no
    int hess_n_orph = -1;             //   block reaches (hess_n_orph of them; -1: no fused assembly for this handle)

    // workspaces sized for max_batch (batch_workspaces, nempc_api.hip, names the ones nempc_reserve empties)
    DevBuf<> d_tiles_ws;         // (Bmax,H,nx,nin) when the caller does not ask for tiles
    DevBuf<> d_g_ws;             // (Bmax,m) when the caller does not ask for g
    DevBuf<> d_valu_ws;          // scratch of the generic row kernel
    DevBuf<> d_hess_ws;          // (Bmax,H,nin,nin) per-row Lagrangian blocks
    DevBuf<> d_kkt_grad;         // (Bmax,n) objective gradient of nempc_kkt_residual's evaluation (tiles / g: the two above)
    DevBuf<double> d_kkt_bounds;             // (2,n) doubles: lb | ub of the last nempc_kkt_residual, +-inf kept
    std::vector<double> kkt_bounds_host;     // ... as last uploaded (empty: nothing uploaded yet)
    DevBuf<> d_sens_ws;                      // nempc_sensitivity (plain models), doubles: gains | value matrices | Sigma | scratch (sens_ws_doubles)
    DevBuf<> d_kktsolve_ws;                  // nempc_kkt_solve, doubles: per-problem global working sets, when its plan needs them
                                             //   (allocated and grown by the call itself, kernels_kktsolve.hip)
    DevBuf<> d_wgrad_ws;                     // nempc_weight_grad: factor matrices | sweep scratch | slabs | kept-problem list
                                             //   (allocated and grown by the call itself, kernels_wgrad.hip)
    DevBuf<> d_egrad_ws;                     // nempc_extra_grad: s', s'' z. of the resident workgroups, when its plan keeps them
                                             //   outside LDS (allocated by the call itself, kernels_egrad.hip)
    DevBuf<> d_rk4_stage;        // RK4 Hessian pipeline (allocated on first use): (Bmax*H, 4, nin + 2*nx*nin) stage records,
    DevBuf<> d_rk4_nu;           //   (Bmax*H, 4, nx) stage multipliers,
    DevBuf<> d_rk4_ht;           //   (Bmax*H, 4, nin, nin) contracted stage Hessians
    DevBuf<long long> d_dbg;     // diagnostic builds only
    bool layered = false;        // rows through the layer-at-a-time GEMM pipeline (kernels_layered.hip) instead of rows_valu_kernel
    DevBuf<> d_layered_ws;          // its chunk workspace (allocated on first use)
    long long layered_chunk_rows = 0;
    DevBuf<> d_layered_hws;         // chunk workspace of its Hessian sweeps (allocated on first use)
    long long layered_hess_chunk_rows = 0;
    bool layered_hess = false;          // a register-resident (MFMA) handle whose Lagrangian blocks come from the layered sweeps (mfma_hess_on_layered)
    DevBuf<> d_layered_pairs;           // (dout[0], nin (nin + 1) / 2): W_0[p][n] W_0[q][n], p >= q (layer 0's curvature term)
    bool layered_pairs_valid = false;
    void* solver_ws = nullptr;   // solver.hip
    void* comm = nullptr;        // comm.hip: RCCL communicator of the u0 all-gather
    mutable int last_row_kernel = ROW_NONE;    // RowKernel (mfma_plan.h) of the most recent row launch (nempc_last_row_kernel)
    mutable int last_hess_kernel = HESS_NONE;  // HessKernel [+ HESS_IN_RK4] of the most recent Lagrangian blocks (nempc_last_hess_kernel)
    mutable int last_dense_writer = 0;  // DenseWriter (post_plan.h) of the most recent nempc_eval (nempc_last_dense_writer)
    mutable int last_lq_kernel = LQ_NONE;            // LqKernel of the most recent solve's plan (nempc_last_lq_kernel)
    mutable int last_rollout_kernel = ROLLOUT_NONE;  // RolloutKernel of the most recent roll-out (nempc_last_rollout_kernel)
    int last_egrad_kernel = 0;                       // EgradKernel (egrad_plan.h) of the most recent nempc_extra_grad
};

// Dynamic LDS above 64 KiB needs hipFuncAttributeMaxDynamicSharedMemorySize, which is a per-device property of the
// kernel: remember the largest size configured per (device, kernel) so the attribute call stays off the hot path.
// Returns hipSuccess when nothing had to be done.
hipError_t ensure_dynamic_lds(const void* kernel, size_t bytes);

// ---- kernels_valu.hip : generic thread-per-row kernel
size_t valu_workspace_elems(const Handle& h);
int ensure_valu_ws(Handle& h);          // generic kernels' scratch, allocated on first need (kernels_valu.hip)
int layered_reserve(Handle& h);         // layered path: both chunk workspaces + pair table (kernels_layered.hip)
int launch_rows_valu(Handle& h, int B, const void* Z, const void* X0, void* g, void* tiles, hipStream_t s);
int launch_rowhess_valu(Handle& h, int B, const void* Z, const void* X0, const void* lambda, void* blocks,
                        hipStream_t s);

// ---- kernels_layered.hip : layer-at-a-time matrix-core path for wide / deep / mixed-activation networks
bool layered_supported(const Handle& h);
int launch_rows_layered(Handle& h, int B, const void* Z, const void* X0, void* g, void* tiles, hipStream_t s);
int launch_rowhess_layered(Handle& h, int B, const void* Z, const void* X0, const void* lambda, void* blocks, hipStream_t s);
int launch_rowhess_layered_direct(Handle& h, long long nrows, const void* stage, int stride, const void* nu, void* out, hipStream_t s);
int launch_rows_layered_stages(Handle& h, int B, const void* Z, const void* X0, void* g, void* tiles, void* stage_out, int stage_stride,
                               hipStream_t s);
// kernels_rk4hess.hip: the RK4 pipeline with the layered launches as steps 1 and 3
int launch_rowhess_rk4_layered(Handle& h, int B, const void* Z, const void* X0, const void* lambda, void* blocks, hipStream_t s,
                               void* g_out, void* tiles_out);

// ---- kernels_rollout.hip : forward simulation x_t = Phi(x_{t-1}, u_t), serial in t, parallel in B
bool rollout_mfma_supported(const Handle& h);
// which: 0 by shape, 1 generic, 2 matrix-core (NEMPC_EUNSUPPORTED when the shape is outside it)
int launch_rollout(Handle& h, int B, const void* X0, void* Z, int which, hipStream_t s);

// ---- kernels_mfma.hip : matrix-core row kernel
bool mfma_supported(const Handle& h);
bool mfma_slower_than_layered(const Handle& h);    // AUTO prefers the layered path (kernels_mfma.hip)
bool mfma_hess_on_layered(const Handle& h);        // AUTO: rows on the register-resident kernels, Lagrangian blocks on the layered sweeps
int mfma_pack_weights(Handle& h, const double* const* W, const double* const* b);
// What a matrix-core launch writes, null = not asked for.  The entry points plan (mfma_plan.h), fill the kernel parameters and
// launch what the plan names; `covers` (may be null) receives the plan's COVERS_* mask: what is left over (assembly, post,
// objective) is the caller's.  NEMPC_EUNSUPPORTED (nothing launched, no error message) means "the plan says not ours", nothing else.
struct RowsOut {
    void *g = nullptr, *tiles = nullptr;    // defects; compact tiles (null with need_tiles: the handle's workspace)
    bool need_tiles = false;                // an assembly launch behind this one reads the tiles
    void *jac = nullptr, *sparse = nullptr, *f = nullptr, *grad = nullptr;
    bool jac_resident = false;              // jac's structural zeros and constants are in place (nempc_jac_dense_resident)
    void* stage_out = nullptr;              // RK4 Hessian pipeline: stage records, stage_stride elements each
    int stage_stride = 0;
    void* gn_hvals = nullptr;               // Gauss-Newton tril values with weights gn_w (null = ones) and gn_sigma
    const void *gn_w = nullptr, *gn_sigma = nullptr;
};
struct HessOut {
    void* blocks = nullptr;                           // (B, H, nin, nin), or the contracted stage Hessians in direct mode
    void* hvals = nullptr;                            // tril values with sigma, and nothing else asked for
    const void* sigma = nullptr;
    void *ev_g = nullptr, *ev_tiles = nullptr;        // blocks + first-order evaluation of the same rows (batched solver)
    const void *xi_direct = nullptr, *lam_direct = nullptr;   // direct mode (RK4 pipeline): vdiv records of xi_stride elements per row
    int xi_stride = 0, vdiv = 1;
};
const MfmaKnobs& mfma_knobs();
MfmaRowsPlan mfma_plan_rows(const Handle& h, int B, const RowsOut& out);
MfmaHessPlan mfma_plan_hess(const Handle& h, int B, const HessOut& out);
int launch_rows_mfma(Handle& h, int B, const void* Z, const void* X0, const RowsOut& out, hipStream_t s, unsigned* covers = nullptr);
int launch_rowhess_mfma(Handle& h, int B, const void* Z, const void* X0, const void* lambda, const HessOut& out, hipStream_t s,
                        unsigned* covers = nullptr);

// ---- kernels_rk4hess.hip : RK4 Lagrangian blocks on the matrix cores (stage records -> stage multipliers ->
//      contracted network Hessians of the four stage inputs -> congruence sum)
bool rk4hess_supported(const Handle& h);     // a wave's slice of the congruence step fits the device's LDS (else: generic kernel)
int launch_rowhess_rk4_mfma(Handle& h, int B, const void* Z, const void* X0, const void* lambda, void* blocks,
                            hipStream_t s, void* g_out = nullptr, void* tiles_out = nullptr);

// ---- kernels_post.hip : objective, dense / sparse assembly, hessian assembly
int launch_objective(Handle& h, int B, const void* Z, void* f, void* grad, hipStream_t s);   // (the binding's kernel when one is present)
// per-problem objective: row b of Z / f / grad is scored against the bound data of problem prob[b] (null: b itself)
int launch_objective_tracking(Handle& h, int B, const void* Z, void* f, void* grad, const int* prob, hipStream_t s);
int launch_assemble_hess_gn(Handle& h, int B, const void* tiles, const void* w, const void* sigma, void* hvals, void* hdense,
                            hipStream_t s);
// resident: jac's structural zeros and constant entries are in place (nempc_jac_dense_resident, launch_jac_constants): only
// the entries that come from the tiles are written
int launch_jac_constants(Handle& h, int b0, int b1, void* jac, hipStream_t s);   // the -1 / +1 entries of problems [b0, b1)
int launch_assemble_dense(Handle& h, int B, const void* tiles, void* jac, hipStream_t s, bool resident = false);
int launch_assemble_sparse(Handle& h, int B, const void* tiles, void* vals, hipStream_t s);
int launch_post(Handle& h, int B, const void* tiles, void* jac, const void* Z, void* f, void* grad, hipStream_t s,
                bool resident = false);
int launch_post_sparse(Handle& h, int B, const void* tiles, void* vals, const void* Z, void* f, void* grad,
                       hipStream_t s);
int launch_assemble_hess(Handle& h, int B, const void* blocks, const void* sigma, void* hvals, void* hdense,
                         hipStream_t s);
int launch_gn_blocks(Handle& h, int B, const void* tiles, const void* w, void* blocks, hipStream_t s);
// KKT residuals of B primal-dual points from an evaluation's grad / g / tiles (kernels_kkt_impl.h): r (B,4), stat (B,n) or
// null; zl / zu null = zeros; lb / ub (n) DEVICE doubles (+-inf for a missing bound) or null = unbounded
int launch_kkt_residual(Handle& h, int B, const void* Z, const void* grad, const void* g, const void* tiles, const void* lam,
                        const void* zl, const void* zu, const double* lb, const double* ub, void* r, void* stat, hipStream_t s);

// ---- kernels_sens.hip : solution sensitivities dz*/dx0 (nempc_sensitivity)
size_t sens_ws_doubles(const Handle& h, size_t Bmax);   // elements of Handle::d_sens_ws for a batch of Bmax
// tiles (B,H,nx,nin), blocks (B,H,nin,nin) of the point; lam is not needed (it is inside the blocks).  zl / zu null = zeros;
// lb / ub (n) DEVICE doubles or null; outputs as nempc_sensitivity (each may be null), status (B) device
int launch_sensitivity(Handle& h, int B, const void* Z, const void* tiles, const void* blocks, const void* zl, const void* zu,
                       const double* lb, const double* ub, void* dU0, void* dZ, void* dlam, void* gains, int32_t* status,
                       hipStream_t s);

// ---- kernels_kktsolve.hip : KKT solves with caller-supplied right-hand sides (nempc_kkt_solve)
size_t kktsolve_ws_doubles(const Handle& h, size_t Bmax, int nrhs);   // doubles of Handle::d_kktsolve_ws (0: the plan is on-chip)
// as launch_sensitivity, with rz (B,nrhs,n), rg (B,nrhs,H nx) or null and the outputs of nempc_kkt_solve (each may be null).
// Uses Handle::d_sens_ws for the gains, value matrices and Sigma; grows Handle::d_kktsolve_ws (a device synchronisation)
int launch_kkt_solve(Handle& h, int B, const void* Z, const void* tiles, const void* blocks, const void* zl, const void* zu,
                     const double* lb, const double* ub, int nrhs, const void* rz, const void* rg, void* v, void* w, void* gx0,
                     int32_t* status, hipStream_t s);

// ---- kernels_wgrad.hip : gradient with respect to the network's weights (nempc_weight_grad)
long long wgrad_n_params(const Handle& h);
// lam / v both or neither; skip (B) device or null; gtheta (P) is overwritten.  Grows Handle::d_wgrad_ws (a device
// synchronisation) when the plan needs more than it holds
int launch_weight_grad(Handle& h, int B, const void* Z, const void* X0, const void* lam, const void* v, const void* w,
                       const int32_t* skip, void* gtheta, hipStream_t s);

// ---- kernels_egrad.hip : gradient with respect to the extra network inputs (nempc_extra_grad)
// lam / v both or neither; gE (B,H,ne) is overwritten.  Allocates Handle::d_egrad_ws (a device synchronisation) when the plan
// keeps the saved activation derivatives outside LDS
int launch_extra_grad(Handle& h, int B, const void* Z, const void* X0, const void* lam, const void* v, const void* w, void* gE,
                      hipStream_t s);

// ---- solver.hip : batched Gauss-Newton SQP (host driver; its kernels are in solver_args.h and the solver_*_impl.h headers,
// which only solver.hip includes)
// LDS bytes of a workgroup that plan_lq (solver.hip), sens_plan (kernels_sens.hip) and kktsolve_plan (kernels_kktsolve.hip)
// fill with per-problem working sets
constexpr size_t kLqLdsBudget = (size_t)150 * 1024;
// the caller's variable bounds (n host doubles each, null = unbounded) intersected with the handle's box rows on the state
// variables -> lo, hi (n, +-INFINITY for a missing bound).  lo > hi is NEMPC_EINVAL, lo == hi too when `need_interior`;
// `who` names the entry point in the message.
int intersect_bounds(const Handle& h, const double* lb, const double* ub, bool need_interior, const char* who,
                     std::vector<double>& lo, std::vector<double>& hi);
// multipliers the solver hands back (each may be null): lam (B,m), zl / zu (B,n), device, dtype of the handle
struct SolverDuals {
    void *lam = nullptr, *zl = nullptr, *zu = nullptr;
    bool any() const { return lam || zl || zu; }
};
int solver_run(Handle& h, int B, const void* X0, void* Z, const double* lb, const double* ub,
               const nempc_solver_opts& o, int32_t* status_dev, int32_t* iters_host, const SolverDuals& duals, hipStream_t s);
void solver_free(Handle& h);

// ---- comm.hip : RCCL all-gather of the first controls
void comm_free(Handle& h);

}  // namespace nempc
