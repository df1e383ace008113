// Layer-at-a-time matrix-core path (gfx950) for networks the register-resident kernels do not take: hidden widths up to
// 1024, up to NEMPC_MAX_LAYERS dense layers, any activation per layer (the output layer included).
//
// The reference wraps ANY feed-forward Keras model (model/tensorflow.py:8-29,49-51) and differentiates it per row
// (tensorflow.py:53-75).  The fused row kernels of this library keep a network's weight slices in registers, which ends at
// three hidden layers of width 128 with one activation; everything else used to run on the thread-per-row kernel
// (rows_valu_kernel: ~50x slower).  For those networks a dense layer over all B*H rows is a GEMM large enough to stand on
// its own -- (B*H) x width x width -- so the network is walked one layer per launch:
//
//   forward   X_l = s_l(X_{l-1} W_l + b_l),  D_l = s_l'(z_l)                 one GEMM per layer, activation in the epilogue
//   reverse   G_{L-2} = (W_{L-1} e_k s_{L-1}') . D_{L-2}                    seed: all nx cotangents side by side
//             G_{l-1} = (G_l W_l^T) . D_{l-1}                               one GEMM per layer over nx * (B*H) columns
//             J       = G_0 W_0^T                                           skinny: onto the nin inputs
//   integrator algebra (discret.py:27,52-56 / unity.py:29 / rk4.py:69-80,147-159) per row, then the same g / compact-tile
//   outputs as the row kernels; the dense / sparse / objective launches of nempc_eval follow unchanged.
//
// Layout: every activation matrix is stored FEATURE-MAJOR, X^T[feature][row] with a row stride Rp (multiple of 64): the
// 16x16x4 matrix instructions compute Z^T (features x rows) = W^T (features x k) . X^T (k x rows), so a result register is
// 16 consecutive rows of one feature -- a coalesced store -- and the next layer's operand tile is a plain 2-D sub-block of
// X^T: no transposition anywhere, and the weights are used as nempc_set_weights left them (W row-major (in, out) forward,
// W^T row-major (out, in) reverse: d_W / d_Wt of the generic kernel).
//
// GEMM kernel: 256 threads = 4 waves own a 64 (features) x 64 (rows) block, each wave 32 x 32 = 2 x 2 accumulator tiles;
// K in chunks of 16 through double-buffered LDS (global loads of chunk c+1 in flight under the matrix instructions of
// chunk c).  Per chunk and wave: 16 matrix instructions (1024 cycles in fp64), 16 ds_read, 8 global loads.  A v_mfma_f64
// holds the vector pipe for its 64 cycles, so the bound is the matrix pipe; arbitrary M, N, K (edge tiles are
// zero-filled on load and masked on store).
#include <algorithm>
#include <string>

#include "kernels_layered_impl.h"

namespace nempc {

namespace {

LayeredNet layered_net(const Handle& h) {       // (the fields in the struct's order)
    return LayeredNet{h.cfg.nx, h.nin, h.ne, h.nl, h.maxw, h.cfg.integrator, h.num_cus, h.din, h.dout, h.act, h.esz};
}

#define LG_TRY(call)                            \
    do {                                        \
        if (const int rc_ = (call)) return rc_; \
    } while (0)

// every loan of a plan against its region, before the sweep's first launch
int check_loans(std::initializer_list<const LgLoan*> loans) {
    for (const LgLoan* b : loans)
        if (b->used() && !b->fits()) {
            set_error(std::string("layered workspace: ") + b->name + " lent for " + std::to_string(b->rows) + " rows, holds " +
                      std::to_string(b->region.rows));
            return NEMPC_EINVAL;
        }
    return NEMPC_OK;
}

// forward product of layer l over R rows: X_l = s_l(X_{l-1} W_l + b_l); the caller says what is stored
GemmArgs forward_product(const Handle& h, int l, const void* in, int R, long long Rp) {
    GemmArgs a{};
    a.mode = LG_FORWARD; a.act = h.act[l]; a.actp = h.actp[l];
    a.A = in; a.lda = Rp; a.ldd = Rp;
    a.Bw = h.d_W[l].get(); a.ldb = h.dout[l]; a.bias = h.d_b[l].get();
    a.M = R; a.N = h.dout[l]; a.K = h.din[l];
    return a;
}
// reverse product: M columns (cotangent or tangent blocks of Rmod rows side by side) through Bw (K, N)
GemmArgs reverse_product(const void* Bw, int N, int K, long long M, long long Rmod) {
    GemmArgs a{};
    a.mode = LG_REVERSE; a.Bw = Bw; a.ldb = N;
    a.M = (int)M; a.N = N; a.K = K; a.Rmod = Rmod;
    return a;
}
// ... times the derivatives of layer l from its stored matrix D: s' itself, or (dfa) the activation it is formed from
void derivs_from(GemmArgs& a, const Handle& h, int l, bool dfa, void* D, long long Rp) {
    a.D = D; a.ldd = Rp;
    if (dfa) { a.dact = h.act[l]; a.dactp = h.actp[l]; }
}
// ... whose operand the loader forms from layer l's stored matrix Dl and the rows of seedW (SEED; seedDl: s_L', null for 1)
void seed_from(GemmArgs& a, const Handle& h, int l, bool dfa, const void* Dl, long long Rp, const void* seedW, int seed_nx,
               const void* seedDl) {
    a.A = Dl; a.lda = Rp;
    a.seedW = seedW; a.seedDl = seedDl; a.seed_nx = seed_nx;
    if (dfa) { a.sact = h.act[l]; a.sactp = h.actp[l]; }
}
// ... whose result is contracted with Wc (nd columns, row stride ldw) in the epilogue: partial sums per feature block at Jp
void contract_into(GemmArgs& a, const void* Wc, int ldw, int nd, void* Jp, long long ldj, long long stride) {
    a.w0t = Wc; a.ldw0 = ldw; a.nin = nd;
    a.Jp = Jp; a.ldj = ldj; a.jp_stride = stride;
}

// Host driver.  A sweep over the rows of one call is planned before it launches anything (layered_plan.h); Sweep walks the plan
// chunk by chunk, its members being the named steps.  A step's context is the chunk: rows r0 .. r0 + R, every matrix with the
// row stride Rp -- R in whole GEMM blocks (a short batch on a handle sized for a large one does not pay for the columns it
// does not have).  Plan: RowsPlan or HessPlan; of the steps below only those of that sweep are ever instantiated.
template <typename T, typename Plan>
struct Sweep {
    const Handle& h;
    const Plan p;
    T* const ws;
    const hipStream_t s;
    const T* const Z;
    const T* const X0;
    const decltype(Plan::ws)& o = p.ws;     // the workspace layout (a reference into this object: no copies)
    const RowGather gk = h.gather();
    const int nx = h.cfg.nx, nin = h.nin, ne = h.ne, nl = h.nl;
    long long r0 = 0, Rp = 0;
    int R = 0;
    dim3 rb{256}, rg{1};        // a thread per row
    Sweep(const Sweep&) = delete;

    bool next_chunk(long long rows, long long Rc) {       // -> false: the call's rows are done
        r0 += R;
        if (r0 >= rows) return false;
        R = (int)(rows - r0 < Rc ? rows - r0 : Rc);
        Rp = ((long long)R + LG_BM - 1) / LG_BM * LG_BM;
        rg = dim3((unsigned)((R + 255) / 256));
        return true;
    }
    T* at(const LgRegion& r) const { return ws + r.off * (size_t)Rp; }
    static const T* typed(const void* p) { return static_cast<const T*>(p); }
    // the one launch + error check; every argument is converted to the kernel's parameter type (the handle's void pointers too)
    template <typename... P, typename... A>
    int launch(void (*kern)(P...), dim3 grid, dim3 block, A... args) const {
        hipLaunchKernelGGL(kern, grid, block, 0, s, static_cast<P>(args)...);
        NEMPC_HIP(hipGetLastError());
        return NEMPC_OK;
    }

    // ---- forward: hidden layers 0 .. nl-2 (GEMM), output layer nl-1.  One walk for both sweeps (first and dfa are members of
    // either plan); they differ in
    //   e            the stored derivatives: s'' next to s', per layer (Hessian sweeps); null: s' only
    //   sums         where the output contraction's partial sums go (last hidden layer's epilogue); null: no contraction
    //   out_step     the output step runs (the contraction's finish, or the skinny product) -- storing s_L'' at el unless null
    int forward(const LgRegion* e, const LgLoan* sums, bool out_step, const LgRegion* el) const {
        T* const elp = el ? at(*el) : nullptr;
        const T* in = at(o.xi);
        for (int l = 0; l < nl - 1; ++l) {
            T* const out = p.dfa[l] ? at(o.d[l]) : at((l & 1) ? o.x1 : o.x0);
            T* const D = p.dfa[l] ? nullptr : at(o.d[l]);
            T* const E = p.dfa[l] || !e ? nullptr : at(e[l]);
            if (l == 0 && p.first) {
                LG_TRY(launch_first<T>(h.act[0], nin + ne, dim3((unsigned)((R + 63) / 64), (unsigned)lg_fblocks(h.dout[0])), s, gk, nin, ne,
                                       typed(h.d_extra), Z, X0, r0, R, Rp, typed(h.d_W[0].get()), h.dout[0], typed(h.d_b[0].get()), h.act[0],
                                       (T)h.actp[0], out, D, E));
                in = out;
                continue;
            }
            GemmArgs a = forward_product(h, l, in, R, Rp);
            if (l == nl - 2 && sums) {
                // the last hidden layer: its activations go straight into the output layer's contraction (only s' -- or, dfa,
                // the activation itself, through the D slot -- is stored); partial sums per feature block
                a.D = at(o.d[l]); a.E = E; a.store_a = p.dfa[l] ? 1 : 0;
                contract_into(a, h.d_W[nl - 1].get(), nx, nx, at(sums->region), Rp, (long long)nx * Rp);
                LG_TRY((gemm_forward<T, LG_CONTRACT_FORWARD>(h.num_cus, s, a)));
                if (!out_step) return NEMPC_OK;
                return launch(layered_outfinish_kernel<T>, rg, rb, at(sums->region), lg_fblocks(h.dout[l]), a.jp_stride, nx, R, Rp,
                              h.d_b[nl - 1].get(), h.act[nl - 1], h.actp[nl - 1], at(o.f), at(o.dl), elp);
            }
            a.C = out; a.ldc = Rp; a.D = D; a.E = E;
            LG_TRY((gemm_forward<T, LG_CONTRACT_NONE>(h.num_cus, s, a)));
            in = out;
        }
        if (!out_step) return NEMPC_OK;
        return skinny<T>(s, in, Rp, typed(h.d_W[nl - 1].get()), nx, h.din[nl - 1], nx, (long long)R, at(o.f), Rp, typed(h.d_b[nl - 1].get()), 0,
                         h.act[nl - 1], at(o.dl), (T)h.actp[nl - 1], elp);
    }

    // xi: the rows' network inputs (unless layer 0's launch gathers them itself).  RK4 stages add c DT k_{s-1} to the state part;
    // stage != null: from the stage records (direct mode)
    int gather(const T* kprev, T cdt, const T* stage = nullptr, int stage_stride = 0) const {
        if (stage) return launch(layered_hgather_direct_kernel<T>, rg, rb, stage, stage_stride, nin, ne, h.d_extra, r0, R, Rp, at(o.xi));
        if (p.first) return NEMPC_OK;
        return launch(layered_gather_kernel<T>, rg, rb, gk, nin, ne, h.d_extra, Z, X0, r0, R, Rp, at(o.xi), kprev, cdt);
    }

    // reverse, all nx cotangents side by side: column k Rp + r is (cotangent k, row r).  Fused: see RowsPlan::fused_reverse
    int rows_reverse_fused() const {
        const long long ldg = (long long)nx * Rp;
        T* const Jp = p.jac_sums.used() ? at(p.jac_sums.region) : at(o.j);
        for (int l = nl - 3; l >= 0; --l) {
            const bool seed = l == nl - 3, last = l == 0, even = (nl - 3 - l) % 2 == 0;     // products nl-3 .. 0 write g0, g1, g0, ...
            GemmArgs a = reverse_product(h.d_Wt[l + 1].get(), h.dout[l], h.dout[l + 1], ldg, Rp);
            derivs_from(a, h, l, p.dfa[l], at(o.d[l]), Rp);
            if (seed) seed_from(a, h, nl - 2, p.dfa[nl - 2], at(o.d[nl - 2]), Rp, h.d_W[nl - 1].get(), nx, p.lin_skip ? nullptr : at(o.dl));
            else { a.A = at(even ? o.g1 : o.g0); a.lda = ldg; }
            if (last) contract_into(a, h.d_Wt[0].get(), h.din[0], nin, Jp, ldg, (long long)nin * ldg);
            else { a.C = at(even ? o.g0 : o.g1); a.ldc = ldg; }
            LG_TRY(gemm_reverse_fused<T>(s, a, seed, last));
        }
        if (!p.jac_sums.used() || !p.rk4) return NEMPC_OK;      // (Discret / Unity: layered_finish_kernel adds the blocks itself)
        const long long count = (long long)nin * ldg;
        return launch(layered_jreduce_kernel<T>, dim3((unsigned)std::min<long long>((count + 255) / 256, 4096)), dim3(256), Jp,
                      lg_fblocks(h.dout[0]), count, at(o.j), count);
    }
    // ... plain: the seed kernel, one product per layer, the skinny last step onto the inputs
    int rows_reverse_plain() const {
        const long long ldg = (long long)nx * Rp;
        T* G = at(o.g0);
        LG_TRY(launch(layered_seed_kernel<T>, dim3(rg.x, (unsigned)h.dout[nl - 2]), rb, h.d_W[nl - 1].get(), h.dout[nl - 2], nx, at(o.dl),
                      at(o.d[nl - 2]), R, Rp, G, p.dfa[nl - 2] ? h.act[nl - 2] : 0, h.actp[nl - 2]));
        for (int l = nl - 3; l >= 0; --l) {
            // G_l = (W_{l+1} G_{l+1}) . D_l : K = dout[l+1], N = dout[l], operand W_{l+1}^T row-major (out, in) = d_Wt[l+1]
            // the nx blocks of Rp columns are covered as one run of columns
            T* Gn = (G == at(o.g0)) ? at(o.g1) : at(o.g0);
            GemmArgs a = reverse_product(h.d_Wt[l + 1].get(), h.dout[l], h.dout[l + 1], ldg, Rp);
            a.A = G; a.lda = ldg; a.C = Gn; a.ldc = ldg;
            derivs_from(a, h, l, p.dfa[l], at(o.d[l]), Rp);
            a.dactp = h.actp[l];        // (passed whether or not dact is set; read only with it)
            LG_TRY((gemm_ft<T, 1>(s, a)));
            G = Gn;
        }
        // J^T[d][k Rp + r] = sum_o W_0[d][o] G_0[o][.]: operand W_0^T (out, in) = d_Wt[0], only the nin decision inputs
        return skinny<T>(s, G, ldg, typed(h.d_Wt[0].get()), h.din[0], h.dout[0], nin, (long long)(nx - 1) * Rp + R, at(o.j), ldg, nullptr, 2, 0,
                         nullptr, T(0));
    }
    // RK4: the stage's record for the Hessian pipeline (when asked for), then k_s, dk_s and the weighted sums
    int rows_rk4_stage(int st, T cdt, T* stage_out, int stage_stride) const {
        // wide states: dk_{s-1} and dk_s alternate between the two buffers (the threads of every state read dk_{s-1})
        T* const dkc = at((st & 1) ? o.dkn : o.dk);
        T* const dkn = at((st & 1) ? o.dk : o.dkn);
        const T wgt = (st == 0 || st == 3) ? T(1) : T(2);
        if (stage_out && p.wide)
            LG_TRY(launch(layered_stage_record_wide_kernel<T>, dim3(rg.x, (unsigned)nx), rb, st, nx, nin, r0, R, Rp, at(o.xi), at(o.j), dkc,
                          stage_out, stage_stride));
        else if (stage_out)
            LG_TRY(launch(layered_stage_record_kernel<T>, rg, rb, st, nx, nin, r0, R, Rp, at(o.xi), at(o.j), at(o.dk), stage_out,
                          stage_stride));
        if (p.wide)
            return launch(layered_rk4_wide_kernel<T>, dim3(rg.x, (unsigned)nx, (unsigned)nin), rb, st, nx, nin, cdt, wgt, at(o.f), at(o.j),
                          R, Rp, at(o.kprev), at(o.acck), dkc, dkn, at(o.accdk));
        return launch(layered_rk4_kernel<T>, rg, rb, st, nx, nin, cdt, wgt, at(o.f), at(o.j), R, Rp, at(o.kprev), at(o.acck), at(o.dk),
                      at(o.dkn), at(o.accdk));
    }
    // defects, box rows and tiles; network output and Jacobian as they were left: finished, or as feature blocks of partial sums
    int rows_finish(T* g, T* tiles) const {
        const bool jsums = p.jac_sums.used() && !p.rk4, fsums = p.lin_skip;
        const long long jstride = jsums ? (long long)nin * nx * Rp : 0, fstride = fsums ? (long long)nx * Rp : 0;
        return launch(layered_finish_kernel<T>, dim3(rg.x, (unsigned)nx), rb, gk, h.cfg.integrator, h.cfg.DT, nin, Z, X0, r0, R, Rp,
                      fsums ? at(p.out_sums.region) : at(o.f), jsums ? at(p.jac_sums.region) : at(o.j), p.rk4 ? at(o.acck) : nullptr,
                      p.rk4 ? at(o.accdk) : nullptr, g, h.m, h.box ? 1 : 0, tiles, jsums ? lg_fblocks(h.dout[0]) : 1, jstride,
                      fsums ? lg_fblocks(h.dout[nl - 2]) : 0, fstride, h.d_b[nl - 1].get());
    }

    // reverse with the multipliers as the one cotangent: curvature weights w_l of every hidden layer -- and, fuse_l0, layer 0's
    // curvature term from the epilogue of the product that forms q_0
    int hess_cotangents(const T* lam, bool direct) const {
        auto E = [&](int l) { return p.dfa[l] ? at(o.d[l]) : at(o.e[l]); };     // where layer l's s'' comes from
        LG_TRY(launch(layered_hmult_kernel<T>, rg, rb, h.cfg.H, nx, h.m, lam, direct ? 1 : 0, r0, R, Rp, at(o.dl), h.act[nl - 1], at(o.cl),
                      at(o.wl)));
        T* dq = at(o.q0);
        LG_TRY(launch(layered_hseed_kernel<T>, dim3(rg.x, (unsigned)h.dout[nl - 2]), rb, h.d_W[nl - 1].get(), h.dout[nl - 2], nx, at(o.cl),
                      at(o.d[nl - 2]), E(nl - 2), R, Rp, dq, at(o.cw[nl - 2]), p.dfa[nl - 2] ? h.act[nl - 2] : 0, h.actp[nl - 2]));
        for (int l = nl - 3; l >= 0; --l) {
            T* dn = (dq == at(o.q0)) ? at(o.q1) : at(o.q0);
            GemmArgs a = reverse_product(h.d_Wt[l + 1].get(), h.dout[l], h.dout[l + 1], Rp, Rp);
            a.A = dq; a.lda = Rp;
            derivs_from(a, h, l, p.dfa[l], at(o.d[l]), Rp);
            a.E = E(l);
            if (l == 0 && p.fuse_l0) {
                // w_0 = q_0 . E_0 contracted with the pair products
                a.D = E(0);
                a.duse = 1;
                contract_into(a, h.d_layered_pairs.get(), p.npair, p.npair, at(p.l0p_stack.region), Rp, (long long)p.npair * Rp);
                return gemm_ft<T, 1, false, LG_CONTRACT_REVERSE>(s, a);
            }
            a.C = l > 0 ? dn : nullptr; a.C2 = at(o.cw[l]); a.ldc = Rp;
            // (two loads and two stores per element in the epilogue and only B*H columns: the small-launch rule of the
            // forward products applies)
            LG_TRY((gemm_forward<T, LG_CONTRACT_NONE>(h.num_cus, s, a)));
            dq = dn;
        }
        return NEMPC_OK;
    }
    // tangents of all nin inputs side by side (column p Rp + r), contracted layer by layer: folded into the products' epilogues
    // (HessPlan::fold) or through memory.  -> ta: D . P of the last hidden layer, hacc_used: the accumulators hold a term
    int hess_tangents(long long ldt, const T*& ta, bool& hacc_used) const {
        const long long Mt = p.fold ? ldt : (long long)nin * Rp;
        for (int l = 1; l < nl - 1; ++l) {
            T* tn = (ta == at(o.a0)) ? at(o.a1) : at(o.a0);
            const bool need_a = l < nl - 2 || !p.lin_out;     // D_l . P_l feeds the next layer (or the output layer's curvature)
            GemmArgs a = reverse_product(h.d_W[l].get(), h.dout[l], h.din[l], Mt, p.fold ? (long long)R : Rp);
            derivs_from(a, h, l, p.dfa[l], at(o.d[l]), Rp);
            a.C = need_a ? tn : nullptr; a.Craw = p.fold ? nullptr : at(o.P); a.ldc = ldt;
            if (l == 1) seed_from(a, h, 0, p.dfa[0], at(o.d[0]), Rp, h.d_Wt[0].get(), h.din[0], nullptr);     // P_0 = W_0^T, constant
            else { a.A = ta; a.lda = ldt; }
            if (p.fold) {
                // (LG_CONTRACT_HPAIR: the weights w_l with the stride of D, as many inputs as the tile has)
                T* const sums = at(p.l0p_stack.region) + (size_t)p.l0p_at[l] * p.npair * Rp;
                contract_into(a, at(o.cw[l]), 0, 0, sums, Rp, (long long)p.npair * Rp);
                LG_TRY(gemm_hpair<T>(s, a, l == 1, nin));
            } else {
                LG_TRY(l == 1 ? (gemm_ft<T, 1, true, LG_CONTRACT_NONE>(s, a)) : (gemm_ft<T, 1>(s, a)));
                LG_TRY(hcontract<T>(s, at(o.P), ldt, nullptr, 0, at(o.cw[l]), h.dout[l], nin, R, Rp, at(o.hacc), hacc_used));
                hacc_used = true;
            }
            ta = tn;
        }
        return NEMPC_OK;
    }
    // one chunk: forward -- cotangents -- layer-0 term -- tangents -- output-layer term -- finish
    int hess_chunk(const T* lam, const T* stage, int stage_stride, T* blocks) const {
        T* const Hacc = at(o.hacc);
        // forward, every layer's s' and s'' kept (or its activation alone: HessPlan::dfa)
        LG_TRY(gather(nullptr, T(0), stage, stage_stride));
        LG_TRY(forward(o.e, p.contract_out ? &p.out_sums : nullptr, !p.lin_noout, &o.wl));
        LG_TRY(hess_cotangents(lam, stage != nullptr));
        // layer 0: constant tangents W_0^T
        if (!p.fuse_l0) LG_TRY(hcontract<T>(s, nullptr, 0, typed(h.d_W[0].get()), h.dout[0], at(o.cw[0]), h.dout[0], nin, R, Rp, Hacc, false));
        const long long ldt = p.fold ? ((long long)R + 15) / 16 * 16 * nin : (long long)nin * Rp;
        const T* ta = nullptr;
        bool hacc_used = !p.fuse_l0;
        LG_TRY(hess_tangents(ldt, ta, hacc_used));
        if (!p.lin_out) {
            // the output layer's own curvature: P_L = W_L^T (D_{L-2} . P_{L-2}), weights mult . s_L''
            LG_TRY(skinny<T>(s, ta, ldt, typed(h.d_W[nl - 1].get()), nx, h.din[nl - 1], nx, (long long)(nin - 1) * Rp + R, at(o.pl), ldt, nullptr,
                             2, 0, nullptr, T(0)));
            LG_TRY(hcontract<T>(s, at(o.pl), ldt, nullptr, 0, at(o.wl), nx, nin, R, Rp, Hacc, hacc_used));
            hacc_used = true;
        }
        return launch(layered_hfinish_kernel<T>, dim3(rg.x, (unsigned)p.npair), rb, nin, r0, R, Rp, hacc_used ? Hacc : nullptr,
                      p.fuse_l0 ? at(p.l0p_stack.region) : nullptr, p.pblocks, (long long)p.npair * Rp, blocks);
    }
};

template <typename T>
int run_layered(Handle& h, int B, const void* Z, const void* X0, void* g, void* tiles, hipStream_t s, void* stage_out = nullptr,
                int stage_stride = 0) {
    const RowsPlan p = plan_rows(layered_net(h), layered_knobs());
    LG_TRY(check_loans({&p.out_sums, &p.jac_sums}));
    Sweep<T, RowsPlan> c{h, p, h.d_layered_ws.as<T>(), s, static_cast<const T*>(Z), static_cast<const T*>(X0)};
    while (c.next_chunk((long long)B * h.cfg.H, h.layered_chunk_rows)) {
        for (int st = 0; st < (p.rk4 ? 4 : 1); ++st) {
            const T DT = (T)h.cfg.DT, cdt = st == 0 ? T(0) : (st == 3 ? DT : T(0.5) * DT);
            LG_TRY(c.gather(st > 0 ? c.at(p.ws.kprev) : nullptr, cdt));
            LG_TRY(c.forward(nullptr, p.fuse_out ? &p.out_sums : nullptr, !p.lin_skip, nullptr));
            LG_TRY(p.fused_reverse ? c.rows_reverse_fused() : c.rows_reverse_plain());
            if (p.rk4) LG_TRY(c.rows_rk4_stage(st, cdt, static_cast<T*>(stage_out), stage_stride));
        }
        LG_TRY(c.rows_finish(static_cast<T*>(g), static_cast<T*>(tiles)));
    }
    return NEMPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Contracted network Hessian  sum_k mult_k d2 f_k / d xi^2  of every row on the same GEMM kernel (model/tensorflow.py:77-109
// takes tf.hessians per output; contracted with the multipliers as optimizer/ipopt.py:79-80 does).  The layer-wise form of
// rowhess_valu_kernel / net_hessian_contracted (kernels_valu.hip):
//
//     H = sum_l P_l^T diag(w_l) P_l,    P_l = d z_l / d xi  (width_l x nin, pre-activation tangents),
//                                       w_l = q_l . s_l''(z_l),   q_l = d(mult . f) / d a_l
//
//   forward            as the rows path, every layer also stores s''(z) = r2(a) s'(z)                    (GEMMs, R columns)
//   reverse            ONE cotangent (the multipliers): q_{l-1} = W_l (q_l . D_l); the epilogue also writes w_l = q_l . E_l
//                                                                                                         (GEMMs, R columns)
//   tangents           P_0 = W_0^T (constant), P_l = W_l^T (D_{l-1} . P_{l-1}): all nin directions side by side; the first
//                      product forms D_0 . W_0^T in its loader (the SEED form)                         (GEMMs, nin R columns)
//   contraction        per layer, H[p][q][r] += sum_j w_l[j][r] P_l[j][p, r] P_l[j][q, r]: streams P_l once per block pair of
//                      inputs, thread per row, four waves split the features                                (vector unit)
// (2 + nin) GEMM sweeps instead of the 2 + 2 nin of forward-over-reverse.  RK4 models keep the generic kernel for now.

// stage != null: direct mode -- `nrows` rows whose inputs are the stage records' xi and whose multipliers are lam[(row)][nx]
template <typename T>
int run_layered_hess(Handle& h, int B, const void* Z, const void* X0, const void* lam, void* blocks, hipStream_t s,
                     const void* stage = nullptr, int stage_stride = 0, long long nrows = 0) {
    const HessPlan p = plan_hess(layered_net(h), layered_knobs(), stage != nullptr);
    LG_TRY(check_loans({&p.out_sums, &p.l0p_stack}));
    Sweep<T, HessPlan> c{h, p, h.d_layered_hws.as<T>(), s, static_cast<const T*>(Z), static_cast<const T*>(X0)};
    if (p.fuse_l0 && !h.layered_pairs_valid) {
        const dim3 grid((unsigned)((h.dout[0] + 255) / 256));
        LG_TRY(c.launch(layered_pairs_kernel<T>, grid, dim3(256), h.d_W[0].get(), h.dout[0], h.dout[0], h.nin, h.d_layered_pairs.get()));
        h.layered_pairs_valid = true;
    }
    while (c.next_chunk(stage ? nrows : (long long)B * h.cfg.H, h.layered_hess_chunk_rows))
        LG_TRY(c.hess_chunk(static_cast<const T*>(lam), static_cast<const T*>(stage), stage_stride, static_cast<T*>(blocks)));
    return NEMPC_OK;
}

}  // namespace

bool layered_supported(const Handle& h) { return layered_supported(layered_net(h)); }

// rows per chunk from what 6 GB hold: at most 65536, whole GEMM blocks.  At least 4096 up to 16 states / 32 inputs (3.2 GB for
// the Hessian sweeps of 1024 x 32 in fp64 -- the same floor at 1024 x 128 would be 13 GB); wide states -- whose workspaces grow with nx maxw and
// nin maxw per row -- go down to one block of 64 rows instead: a reverse or tangent product's M is nx or nin times the chunk,
// so a short chunk of a wide shape is still a large launch.
static size_t layered_chunk_rows(bool wide, size_t rc_rows, size_t cap) {
    if (rc_rows > 65536) rc_rows = 65536;
    if (wide) rc_rows = rc_rows < LG_BM ? LG_BM : rc_rows / LG_BM * LG_BM;
    else if (rc_rows < 4096) rc_rows = 4096;
    // NEMPC_LAYERED_CHUNK_ROWS: rows per chunk of both workspaces (tests of the chunk loop; read at every sizing)
    if (const int v = env_int("NEMPC_LAYERED_CHUNK_ROWS", 0); v > 0) rc_rows = (size_t)v;
    if (rc_rows > cap) rc_rows = cap;
    return (rc_rows + LG_BM - 1) / LG_BM * LG_BM;
}

// The rows sweep's chunk workspace, or the Hessian sweeps': rows per chunk so that the whole workspace stays near 6 GB (of 288),
// between 4096 and 65536 rows -- the larger the products, the smaller the share of their launch tails (4 x 512, 6/3,
// B*H = 30720 in fp64 is one chunk of 2.3 GB).  Reallocates only when the chunk length changes.
static int layered_prepare(Handle& h, bool hess) {
#ifdef NEMPC_STAMPS
    g_lg_dbg = h.d_dbg.get();         // (diagnostic builds: every launch of the path passes here first)
#endif
    DevBuf<>& ws = hess ? h.d_layered_hws : h.d_layered_ws;
    long long& chunk_rows = hess ? h.layered_hess_chunk_rows : h.layered_chunk_rows;
    const LayeredNet n = layered_net(h);
    const size_t per_row = hess ? layered_hess_offsets(n).total : layered_offsets(n).total;
    const size_t rc_rows = layered_chunk_rows(lg_wide(n), ((size_t)6144 << 20) / (per_row * h.esz), (size_t)h.cfg.max_batch * h.cfg.H);
    const char* const what = hess ? "layered Hessian workspace" : "layered workspace";
    // (with the Hessian workspace, once: layer 0's pair table -- 32 pairs at most, either dtype; the one place that allocates it)
    if (hess && !h.d_layered_pairs) LG_TRY(h.d_layered_pairs.alloc((size_t)h.maxw * 32 * sizeof(double), what));
    if (ws && chunk_rows == (long long)rc_rows) return NEMPC_OK;
    chunk_rows = (long long)rc_rows;
    return ws.alloc(per_row * rc_rows * h.esz, what);
}

// Lagrangian blocks on the GEMM path: Discret / Unity directly, RK4 through the stage pipeline of kernels_rk4hess.hip.
// NEMPC_EUNSUPPORTED: a nonlinear output layer behind a single hidden layer, NEMPC_LAYERED_HESS=0 (A/B knob).
static bool layered_hess_usable(const Handle& h) {
    if (!layered_knobs().hess || !(h.layered || h.layered_hess)) return false;
    return h.nl >= 2 && !(h.nl == 2 && h.act[h.nl - 1] != NEMPC_ACT_LINEAR);
}

// nempc_create / nempc_reserve: both chunk workspaces and the first-layer pair table of the Hessian, so that no callback
// allocates (the layered_prepare calls in the launchers below then find everything in place and return at once)
int layered_reserve(Handle& h) {
    if (h.layered) LG_TRY(layered_prepare(h, false));       // (layered_hess handles: the Hessian workspace only)
    if (layered_hess_usable(h)) {
        LG_TRY(layered_prepare(h, true));
    }
    return NEMPC_OK;
}

// stage != null: direct mode (RK4 pipeline, step 3) -- contracted network Hessians of `nrows` (row, stage) pairs at the records' inputs
static int layered_hess(Handle& h, int B, const void* Z, const void* X0, const void* lam, void* out, hipStream_t s, const void* stage,
                        int stride, long long nrows) {
    if (!layered_hess_usable(h)) return NEMPC_EUNSUPPORTED;
    if (!stage && h.cfg.integrator == NEMPC_RK4) return launch_rowhess_rk4_layered(h, B, Z, X0, lam, out, s, nullptr, nullptr);
    LG_TRY(layered_prepare(h, true));
    h.last_hess_kernel = HESS_LAYERED;
    return h.cfg.dtype == NEMPC_F64 ? run_layered_hess<double>(h, B, Z, X0, lam, out, s, stage, stride, nrows)
                                    : run_layered_hess<float>(h, B, Z, X0, lam, out, s, stage, stride, nrows);
}
int launch_rowhess_layered(Handle& h, int B, const void* Z, const void* X0, const void* lambda, void* blocks, hipStream_t s) {
    return layered_hess(h, B, Z, X0, lambda, blocks, s, nullptr, 0, 0);
}
int launch_rowhess_layered_direct(Handle& h, long long nrows, const void* stage, int stride, const void* nu, void* out, hipStream_t s) {
    return layered_hess(h, 0, nullptr, nullptr, nu, out, s, stage, stride, nrows);
}

// rows with the stage records of the RK4 Hessian pipeline (step 1)
int launch_rows_layered_stages(Handle& h, int B, const void* Z, const void* X0, void* g, void* tiles, void* stage_out, int stage_stride,
                               hipStream_t s) {
    LG_TRY(layered_prepare(h, false));
    h.last_row_kernel = ROW_LAYERED;
    return h.cfg.dtype == NEMPC_F64 ? run_layered<double>(h, B, Z, X0, g, tiles, s, stage_out, stage_stride)
                                    : run_layered<float>(h, B, Z, X0, g, tiles, s, stage_out, stage_stride);
}

int launch_rows_layered(Handle& h, int B, const void* Z, const void* X0, void* g, void* tiles, hipStream_t s) {
    return launch_rows_layered_stages(h, B, Z, X0, g, tiles, nullptr, 0, s);
}

}  // namespace nempc
