// The layered path's plans and workspace loans over a sweep of shapes, without a GPU (tests/test_cabi_cpu.py compiles and runs
// this; it includes nothing of the library but layered_plan.h).  For every shape layered_supported accepts and every setting of
// the switches: (a) every loan a plan schedules fits the region it names, (b) the rows plan's lin_skip is on exactly where the
// condition the driver had inline holds.  Prints the number of plans checked; exit status 1 and the first failures otherwise.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <thread>
#include <vector>

#include "layered_plan.h"

using namespace nempc;

static std::atomic<long long> g_plans{0};
static std::atomic<int> g_failures{0};

static void fail(const char* what, const LayeredNet& n, int setting) {
    if (++g_failures > 10) return;
    std::printf("FAIL %s: widths", what);
    for (int l = 0; l < n.nl - 1; ++l) std::printf(" %d", n.dout[l]);
    std::printf(", nx %d nin %d ne %d integrator %d output act %d, switch setting %d\n", n.nx, n.nin, n.ne, n.integrator, n.act[n.nl - 1],
                setting);
}

static void check_loan(const LgLoan& b, const LayeredNet& n, int setting) {
    if (b.used() && !b.fits()) fail(b.name, n, setting);
}

// the default and each switch at its non-default value(s)
static int knob_settings(LayeredKnobs* k) {
    int c = 1;          // k[0]: the defaults
    k[c++].fuse = false;
    k[c++].dfa = 0;
    k[c++].dfa = 2;
    k[c++].hfold = false;
    k[c++].outskip = false;
    k[c++].first = false;
    k[c++].rm = 2;
    k[c++].rm = 4;
    k[c++].rm_rev = 2;
    k[c++].cot_order = false;
    k[c++].hess = false;
    return c;
}

// lin_skip as run_layered decided it inline before there was a plan
static bool lin_skip_reference(const LayeredNet& n, const LayeredKnobs& k) {
    const int nl = n.nl;
    const bool rk4 = n.integrator == NEMPC_RK4;
    return k.outskip && k.fuse && nl >= 3 && !rk4 && n.act[nl - 1] == NEMPC_ACT_LINEAR && (n.dout[nl - 2] + 63) / 64 * n.nx <= n.maxw;
}

// a network's per-layer arrays next to its view
struct Net : LayeredNet {
    int din_[NEMPC_MAX_LAYERS] = {}, dout_[NEMPC_MAX_LAYERS] = {}, act_[NEMPC_MAX_LAYERS] = {};
    Net() : LayeredNet{} { din = din_; dout = dout_; act = act_; num_cus = 256; esz = 8; }
    Net(const Net&) = delete;
    void finish() {         // input widths and maxw (the widest hidden layer, as nempc_create has it) from the output widths
        maxw = 1;
        for (int l = 0; l < nl; ++l) {
            din_[l] = l == 0 ? nin + ne : dout_[l - 1];
            if (l < nl - 1 && dout_[l] > maxw) maxw = dout_[l];
        }
    }
};

// where the linear-output shortcut parks its sums, as run_layered chose it inline: the activation buffer that the last hidden
// layer's product does not read -- its operand is layer nl-3's output, in d[nl-3] (dfa) or in x0 / x1 by the layer's parity
static const char* lin_skip_region_reference(const LayeredNet& n, const RowsPlan& p) {
    const int l = n.nl - 3;
    const bool in_is_x1 = !p.dfa[l] && (l & 1);
    return in_is_x1 ? "x0" : "x1";
}

static void check_shape(const Net& n, const LayeredKnobs* knobs, int nknobs, long long& plans) {
    if (!layered_supported(n)) return;
    for (int s = 0; s < nknobs; ++s) {
        const RowsPlan p = plan_rows(n, knobs[s]);
        check_loan(p.out_sums, n, s);
        check_loan(p.jac_sums, n, s);
        if (p.lin_skip != lin_skip_reference(n, knobs[s])) fail("lin_skip", n, s);
        if (p.lin_skip && !(p.out_sums.used() && p.out_sums.region.rows == (size_t)n.maxw &&
                            std::string(p.out_sums.name) == lin_skip_region_reference(n, p) &&
                            p.out_sums.region.off == (p.out_sums.name[1] == '0' ? p.ws.x0.off : p.ws.x1.off)))
            fail("lin_skip's loan", n, s);
        for (int direct = 0; direct < 2; ++direct) {
            const HessPlan q = plan_hess(n, knobs[s], direct != 0);
            check_loan(q.out_sums, n, s);
            check_loan(q.l0p_stack, n, s);
        }
        plans += 3;
    }
}

static const int WIDTHS[] = {1, 3, 8, 11, 12, 16, 63, 64, 65, 128, 130, 1024};
constexpr int NW = sizeof(WIDTHS) / sizeof(WIDTHS[0]);

// every shape with `hidden` hidden layers whose widths are combination wi (a number of `hidden` digits to the base NW)
static void check_widths(int hidden, int wi, const LayeredKnobs* knobs, int nknobs, long long& plans) {
    for (int nx : {1, 2, 7, 12, 16, 17, 64})
        for (int nu : {1, 4, 16, 64})
            for (int ne : {0, 3})
                for (int integ : {NEMPC_DISCRET, NEMPC_UNITY, NEMPC_RK4})
                    for (int out_act : {NEMPC_ACT_LINEAR, NEMPC_ACT_TANH}) {
                        Net n;
                        n.nx = nx; n.nin = nx + nu; n.ne = ne; n.nl = hidden + 1; n.integrator = integ;
                        if (n.nin > 128) continue;
                        // hidden activations: tanh (its s' follows from the activation), and softplus (it does not) on the layers
                        // the combination's number picks -- all-tanh, all-softplus and mixed networks all occur
                        for (int l = 0, w = wi; l < hidden; ++l, w /= NW) {
                            n.dout_[l] = WIDTHS[w % NW];
                            n.act_[l] = ((wi + nx) >> l) & 1 ? NEMPC_ACT_SOFTPLUS : NEMPC_ACT_TANH;
                        }
                        n.dout_[hidden] = nx; n.act_[hidden] = out_act;
                        n.finish();
                        check_shape(n, knobs, nknobs, plans);
                    }
}

int main() {
    LayeredKnobs knobs[16];
    const int nknobs = knob_settings(knobs);
    // (the width combinations dealt round-robin to the machine's threads: 7 million shapes x 12 settings x 3 plans)
    const int nthreads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    auto sweep = [&](int tid) {
        long long plans = 0;
        for (int hidden = 1, combos = NW; hidden <= 4; ++hidden, combos *= NW)
            for (int wi = tid; wi < combos; wi += nthreads) check_widths(hidden, wi, knobs, nknobs, plans);
        g_plans += plans;
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < nthreads; ++t) pool.emplace_back(sweep, t);
    for (std::thread& t : pool) t.join();
    // the two bottleneck shapes either side of the bound: two layers of 11 with 12 states do not fit (12 rows of sums, 11 of room)
    for (int w : {11, 12}) {
        Net n;
        n.nx = 12; n.nin = 13; n.nl = 3; n.integrator = NEMPC_DISCRET;
        n.dout_[0] = n.dout_[1] = w; n.dout_[2] = 12;
        n.act_[0] = n.act_[1] = NEMPC_ACT_TANH; n.act_[2] = NEMPC_ACT_LINEAR;
        n.finish();
        if (plan_rows(n, knobs[0]).lin_skip != (w == 12)) fail("lin_skip at the bottleneck bound", n, 0);
    }
    std::printf("%lld plans checked, %d failures\n", g_plans.load(), g_failures.load());
    return g_failures.load() ? 1 : 0;
}
