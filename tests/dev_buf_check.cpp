// Host check of csrc/dev_buf.h: the raw functions on malloc / free with a live-allocation counter, a log of the order they were
// called in, and switches that fail the next allocation(s) or the next synchronisation.  Built with AddressSanitizer /
// UndefinedBehaviorSanitizer and run on its own (test_dev_buf_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "dev_buf.h"
#include "nempc.h"

static std::set<void*> g_live;      // what the raw allocator handed out and has not seen back
static int g_allocs = 0, g_frees = 0, g_syncs = 0;
static int g_fail_at = 0;           // > 0: that allocation from now (1 = the next one) fails
static bool g_fail_sync = false;    // the next synchronisation fails
static std::string g_log;           // 's'ynchronisation, 'f'ree, 'a'llocation ('A': a failed one), in call order
static const char* g_last_what = "";

namespace nempc {
int dev_raw_sync() {
    ++g_syncs;
    g_log += 's';
    if (g_fail_sync) { g_fail_sync = false; return NEMPC_EHIP; }
    return NEMPC_OK;
}
int dev_raw_alloc(void** p, std::size_t bytes, const char* what) {
    *p = nullptr;
    g_last_what = what;
    if (bytes == 0) { std::printf("FAIL: raw allocation of 0 bytes\n"); std::exit(2); }
    if (g_fail_at > 0 && --g_fail_at == 0) { g_log += 'A'; return NEMPC_ENOMEM; }
    g_log += 'a';
    *p = std::malloc(bytes);
    std::memset(*p, 0xab, bytes);   // (the whole size is ours to write)
    g_live.insert(*p);
    ++g_allocs;
    return NEMPC_OK;
}
void dev_raw_free(void* p) {
    if (!g_live.erase(p)) { std::printf("FAIL: free of an address that is not live\n"); std::exit(2); }
    std::free(p);
    g_log += 'f';
    ++g_frees;
}
}  // namespace nempc

using nempc::DevBuf;

static int g_checks = 0, g_failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) { ++g_failures; std::printf("FAIL line %d: %s\n", __LINE__, #cond); } \
    } while (0)

static void construction_and_destruction() {
    {
        DevBuf<> a;
        CHECK(!a && a.get() == nullptr && a.bytes() == 0);
        a.reset();                          // (an empty buffer: nothing to free)
        CHECK(g_frees == 0);
        CHECK(a.alloc(100, "a") == NEMPC_OK);
        CHECK(a && a.bytes() == 100 && g_live.size() == 1 && std::strcmp(g_last_what, "a") == 0);
        a.as<unsigned char>()[99] = 1;
        DevBuf<double> d;
        CHECK(d.alloc(3 * sizeof(double), "d") == NEMPC_OK);
        d.get()[2] = 1.5;
        CHECK(d.as<double>() == d.get() && (void*)d.as<char>() == (void*)d.get());
        CHECK(g_live.size() == 2);
    }
    CHECK(g_live.empty() && g_allocs == 2 && g_frees == 2);
}

static void zero_bytes_have_an_address() {
    DevBuf<> a, b;
    CHECK(a.alloc(0, "a") == NEMPC_OK && b.alloc(0, "b") == NEMPC_OK);
    CHECK(a && b && a.get() != b.get() && a.bytes() == 0 && b.bytes() == 0);
    CHECK(g_live.size() == 2);
    a.reset();
    CHECK(!a && g_live.size() == 1);
}

static void alloc_over_a_held_buffer() {
    DevBuf<> a;
    CHECK(a.alloc(64, "a") == NEMPC_OK);
    void* const first = a.get();
    const int frees = g_frees;
    CHECK(a.alloc(128, "a") == NEMPC_OK);
    CHECK(g_frees == frees + 1 && !g_live.count(first) && g_live.size() == 1 && a.bytes() == 128);
    a.reset();
    a.reset();
    CHECK(g_frees == frees + 2 && g_live.empty() && !a && a.bytes() == 0);
}

static void ensure_grows_only() {
    DevBuf<> a;
    const int syncs = g_syncs, allocs = g_allocs;
    g_log.clear();
    CHECK(a.ensure(0, "a") == NEMPC_OK && !a && g_allocs == allocs && g_syncs == syncs);   // nothing needed: nothing done
    CHECK(a.ensure(256, "a") == NEMPC_OK && g_syncs == syncs + 1);                          // the first allocation synchronises too
    CHECK(g_log == "sa");
    void* const p = a.get();
    CHECK(a.ensure(256, "a") == NEMPC_OK && a.ensure(10, "a") == NEMPC_OK && a.get() == p);
    CHECK(g_allocs == allocs + 1 && g_syncs == syncs + 1 && a.bytes() == 256 && g_log == "sa");
    CHECK(a.ensure(257, "a") == NEMPC_OK && g_allocs == allocs + 2 && g_syncs == syncs + 2 && a.bytes() == 257);
    CHECK(g_log == "sasfa");                // growing: the synchronisation, then the free of the old one, then the allocation
    CHECK(!g_live.count(p) && g_live.size() == 1);
    void* const q = a.get();
    g_fail_sync = true;                     // a failed synchronisation: its code, and the buffer as it was
    CHECK(a.ensure(1000, "a") == NEMPC_EHIP && a.get() == q && a.bytes() == 257 && g_live.count(q) && g_log == "sasfas");
    g_fail_at = 1;                          // a failed allocation behind a good synchronisation: empty
    CHECK(a.ensure(1000, "a") == NEMPC_ENOMEM && !a && a.bytes() == 0 && g_live.empty() && g_log == "sasfassfA");
    g_log.clear();
    CHECK(a.alloc(8, "a") == NEMPC_OK && a.alloc(9, "a") == NEMPC_OK && g_log == "afa");    // (alloc does not synchronise)
}

static void a_failed_alloc_leaves_it_empty() {
    DevBuf<> a;
    CHECK(a.alloc(32, "a") == NEMPC_OK);
    void* const old = a.get();
    g_fail_at = 1;
    CHECK(a.alloc(64, "a") == NEMPC_ENOMEM);
    CHECK(!a && a.get() == nullptr && a.bytes() == 0 && !g_live.count(old) && g_live.empty());
    g_fail_at = 1;
    CHECK(a.ensure(64, "a") == NEMPC_ENOMEM && !a && a.bytes() == 0);
    CHECK(a.alloc(64, "a") == NEMPC_OK && a && g_live.size() == 1);                       // (usable again)
}

static void moves() {
    DevBuf<> a;
    CHECK(a.alloc(40, "a") == NEMPC_OK);
    void* const pa = a.get();
    DevBuf<> b(std::move(a));
    CHECK(!a && a.bytes() == 0 && b.get() == pa && b.bytes() == 40 && g_live.size() == 1);
    DevBuf<> c;
    CHECK(c.alloc(24, "c") == NEMPC_OK);
    void* const pc = c.get();
    const int frees = g_frees;
    c = std::move(b);                       // what c held is freed once, b is empty
    CHECK(g_frees == frees + 1 && !g_live.count(pc) && c.get() == pa && c.bytes() == 40 && !b && g_live.size() == 1);
    DevBuf<>& same = c;
    c = std::move(same);                    // self-move: untouched
    CHECK(g_frees == frees + 1 && c.get() == pa && c.bytes() == 40 && g_live.count(pa));
    c = DevBuf<>();                         // move from an empty one: freed
    CHECK(!c && g_live.empty());
}

static void an_array_goes_out_of_scope() {
    {
        DevBuf<> layers[8];
        for (int l = 0; l < 8; ++l) CHECK(layers[l].alloc(16 * (l + 1), "layer") == NEMPC_OK);
        CHECK(g_live.size() == 8);
        layers[3].reset();
        CHECK(g_live.size() == 7);
    }
    CHECK(g_live.empty());
}

// nempc_set_weights: a layer's three new buffers first, into the handle only when all of them stand
static int replace_three(DevBuf<>& W, DevBuf<>& Wt, DevBuf<>& b, unsigned char fill) {
    DevBuf<> nW, nWt, nb;
    int rc;
    if ((rc = nW.alloc(48, "W"))) return rc;
    if ((rc = nWt.alloc(48, "Wt"))) return rc;
    if ((rc = nb.alloc(8, "b"))) return rc;
    std::memset(nW.get(), fill, 48); std::memset(nWt.get(), fill, 48); std::memset(nb.get(), fill, 8);
    W = std::move(nW); Wt = std::move(nWt); b = std::move(nb);
    return NEMPC_OK;
}

static void build_three_then_move_in() {
    DevBuf<> W, Wt, b;
    CHECK(replace_three(W, Wt, b, 1) == NEMPC_OK && g_live.size() == 3);
    void* const p[3] = {W.get(), Wt.get(), b.get()};
    for (int fail_at = 1; fail_at <= 3; ++fail_at) {
        g_fail_at = fail_at;
        CHECK(replace_three(W, Wt, b, 9) == NEMPC_ENOMEM);
        g_fail_at = 0;
        CHECK(W.get() == p[0] && Wt.get() == p[1] && b.get() == p[2] && g_live.size() == 3);
        CHECK(g_live.count(p[0]) && g_live.count(p[1]) && g_live.count(p[2]));
        CHECK(W.as<unsigned char>()[47] == 1 && Wt.as<unsigned char>()[0] == 1 && b.as<unsigned char>()[7] == 1);
    }
    CHECK(replace_three(W, Wt, b, 2) == NEMPC_OK && g_live.size() == 3);
    CHECK(!g_live.count(p[0]) && !g_live.count(p[1]) && !g_live.count(p[2]) && W.as<unsigned char>()[47] == 2);
}

int main() {
    void (*const cases[])() = {construction_and_destruction, zero_bytes_have_an_address, alloc_over_a_held_buffer, ensure_grows_only,
                               a_failed_alloc_leaves_it_empty, moves, an_array_goes_out_of_scope, build_three_then_move_in};
    int ncases = 0;
    for (auto f : cases) {
        f();
        ++ncases;
        CHECK(g_live.empty());              // every case gives back what it took
        CHECK(g_allocs == g_frees);
    }
    std::printf("%d cases, %d checks, %d failures\n", ncases, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
