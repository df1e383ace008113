// csrc/egrad_plan.h on the CPU: widths 1 .. 1024, both dtypes, 1 .. 8 layers, RK4 or not, several nx / n_extra / compute-unit
// counts.  For every plan, laid out exactly as kernels_egrad.hip lays it out:
//   * lanes is 1, 16 or 64 from the widest layer, and no group's LDS block reaches into the next one's: the largest LDS
//     element a group touches is below the smallest of the next group, and the last one is inside lds_bytes;
//   * lds_bytes <= EG_LDS_BUDGET when SAVE is in LDS, <= EG_LDS_MAX always (every shape swept here fits);
//   * the padded stride puts the two groups of a 32-lane half 16 banks apart;
//   * SAVE in the workspace: the regions of (workgroup, group) pairs are disjoint (first and last slot of every region of the
//     first workgroups and of the last one, sorted), inside egrad_ws_elems, and the whole stays within EG_WS_BYTES unless one
//     workgroup's region alone is larger;
//   * the grid covers every row (grid stride) and never exceeds the cap.
// Built with -fsanitize=address,undefined and run by tests/test_extra_grad_cpu.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "egrad_plan.h"

using namespace nempc;

static long long failures = 0, plans = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            if (++failures < 20) std::printf("FAIL line %d: %s\n", __LINE__, #c); \
        }                                                                \
    } while (0)

static void check(const EgradShape& s, long long cap_rows) {
    const EgradPlan p = egrad_make_plan(s);
    ++plans;
    int maxdim = 0;
    long long outs = 0;
    for (int l = 0; l < s.nl; ++l) {
        maxdim = std::max(maxdim, std::max(s.din[l], s.dout[l]));
        outs += s.dout[l];
    }
    CHECK(p.maxdim == maxdim);
    CHECK(p.lanes == (maxdim <= 8 ? 1 : (maxdim <= 64 ? 16 : 64)) && p.rows_per_wg * p.lanes == 64);
    CHECK(p.x_elems == 4ll * maxdim + 4ll * s.nx + s.ne && p.save_elems == 2ll * s.nstage * outs);
    const long long per_row = p.x_elems + (p.save_in_lds ? p.save_elems : 0);
    // LDS: element index of slot q of group g, as the kernel forms it
    const long long sl = p.lanes == 1 ? 64 : 1;
    auto lds_at = [&](int g, long long q) { return (p.lanes == 1 ? (long long)g : g * p.stride) + q * sl; };
    const int groups = p.rows_per_wg;
    if (p.lanes == 1) {
        CHECK(p.stride == per_row);
        CHECK(lds_at(63, per_row - 1) < (long long)(p.lds_bytes / s.esz));
        CHECK(lds_at(0, 1) - lds_at(0, 0) == 64);          // lane i on bank i of every slot
    } else {
        CHECK(p.stride >= per_row);
        for (int g = 0; g + 1 < groups; ++g) CHECK(lds_at(g, per_row - 1) < lds_at(g + 1, 0));
        CHECK(lds_at(groups - 1, per_row - 1) < (long long)(p.lds_bytes / s.esz));
        CHECK((p.stride * (long long)(s.esz / 4)) % 32 == 16);
        CHECK(p.stride - per_row < 32);
    }
    CHECK(p.fits && p.lds_bytes <= EG_LDS_MAX);
    if (p.save_in_lds) CHECK(p.lds_bytes <= EG_LDS_BUDGET);
    CHECK(p.code == (p.lanes == 1 ? 1 : (p.lanes == 16 ? 2 : 3)) + (p.save_in_lds ? 0 : 4));
    // grid
    for (long long rows : {1ll, 63ll, 64ll, 65ll, cap_rows}) {
        if (rows > cap_rows) continue;
        const long long g = egrad_grid(p, rows);
        CHECK(g >= 1 && g <= p.max_wgs && g <= (rows + p.rows_per_wg - 1) / p.rows_per_wg);
        CHECK(g <= egrad_grid(p, cap_rows));               // the workspace of the largest call serves every call
    }
    // workspace
    const long long ws = egrad_ws_elems(p, cap_rows);
    if (p.save_in_lds) {
        CHECK(ws == 0 && p.wg_ws_elems == 0);
        return;
    }
    const long long grid = egrad_grid(p, cap_rows);
    CHECK(p.wg_ws_elems == p.save_elems * p.rows_per_wg && ws == grid * p.wg_ws_elems);
    CHECK(ws * (long long)s.esz <= EG_WS_BYTES || grid == 1);
    std::vector<std::pair<long long, long long>> span;      // [first, last] element of a (workgroup, group) region
    std::vector<long long> wgs = {0, 1, grid - 1};
    for (long long wg : wgs) {
        if (wg < 0 || wg >= grid) continue;
        for (int g = 0; g < groups; ++g) {
            const long long a = egrad_ws_offset(p, wg, g, 0), b = egrad_ws_offset(p, wg, g, p.save_elems - 1);
            CHECK(a >= wg * p.wg_ws_elems && b < (wg + 1) * p.wg_ws_elems && b < ws && a <= b);
            if (p.lanes > 1) span.push_back({a, b});
            else CHECK(a % 64 == g && b % 64 == g);          // slot-major: a lane's slots are the residue class of the lane
        }
    }
    std::sort(span.begin(), span.end());
    span.erase(std::unique(span.begin(), span.end()), span.end());      // (grid < 3: a workgroup listed twice)
    for (size_t i = 0; i + 1 < span.size(); ++i) CHECK(span[i].second < span[i + 1].first);
}

int main() {
    const int widths[] = {1, 2, 7, 8, 9, 15, 16, 17, 20, 63, 64, 65, 100, 128, 144, 255, 256, 511, 512, 1000, 1023, 1024};
    for (size_t esz : {(size_t)4, (size_t)8})
        for (int nstage : {1, 4})
            for (int nl = 1; nl <= 8; ++nl)
                for (int wd = 1; wd <= 1024; ++wd) {
                    // every width with one geometry, the listed widths with all of them
                    const bool listed = std::find(std::begin(widths), std::end(widths), wd) != std::end(widths);
                    for (int nx : {1, 6, 64, 1024})
                        for (int ne : {1, 5, 300})
                            for (int cus : {1, 256}) {
                                if (!listed && !(nx == 6 && ne == 5 && cus == 256)) continue;
                                EgradShape s{};
                                s.nl = nl; s.nstage = nstage; s.nx = nx; s.ne = ne; s.num_cus = cus; s.esz = esz;
                                const int nin = std::min(1024, nx + 3 + ne);
                                for (int l = 0; l < nl; ++l) {
                                    s.din[l] = l == 0 ? nin : wd;
                                    s.dout[l] = l == nl - 1 ? nx : wd;
                                }
                                check(s, 1);
                                check(s, 1024ll * 30);
                            }
                }
    std::printf("%lld plans checked, %lld failures\n", plans, failures);
    return failures ? 1 : 0;
}
